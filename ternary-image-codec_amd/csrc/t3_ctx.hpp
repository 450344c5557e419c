// t3_ctx.hpp — the library context (one per GPU, t3_api.cpp) and the helpers the host translation units share (the pure ones: t3_host.hpp).
// Host code only: t3_api*.cpp include it, no .hip file does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/t3hip.h"
#include "t3_device.h"
#include "t3_host.hpp"

namespace t3 {

struct RsTables; struct FxTables; struct QuantTables;

template <class T> void free_dev(T*& p) { if (p) (void)hipFree((void*)p); p = nullptr; }
template <class T> void free_pinned(T*& p) { if (p) (void)hipHostFree((void*)p); p = nullptr; }

struct LutImage { uint32_t* d_img = nullptr; uint32_t bytes = 0; uint32_t k_off[4] = {0, 0, 0, 0}; uint32_t* d_afrag = nullptr; };

// Device tables of the decode half (t3_api_decode.cpp): the field tables decode_init builds, then the tables of one code, built on
// first use under Ctx::tab_mu.  Arrays [4] are indexed by k index (k = 24, 22, 20, 18).
struct DecodeTables {
    FxTables* fxtab = nullptr;                 // field tables of the two-kernel FIXED decoder
    uint8_t* fma = nullptr;                    // fma[x][y][a] = a + x y: one table read per multiply-accumulate of the corrector
    uint32_t* synd_T = nullptr; uint32_t* synd_T16 = nullptr;   // descramble + trit expansion table of the syndrome MFMA, 32 / 16 bank copies
    uint8_t* fx2_small = nullptr;              // log / exp / inverse byte tables + fold tables of the fused decoders
    uint32_t* synd_lut[4] = {};                // syndrome LUT of the two-kernel decoder (synd_lut_bytes(k), t3_dec_plan.hpp)
    uint32_t* roots[4] = {};                   // the Chien search (OLD:611-623) of every locator, tabulated
    uint32_t* synd_afrag[4] = {};              // A operand of the syndrome MFMA (t3_host.hpp build_mfma_syndrome)
    void release() {
        free_dev(fxtab); free_dev(fma); free_dev(synd_T); free_dev(synd_T16); free_dev(fx2_small);
        for (int i = 0; i < 4; ++i) { free_dev(synd_lut[i]); free_dev(roots[i]); free_dev(synd_afrag[i]); }
    }
};
// Device tables of the CRC-32 / frame record unit (t3_api_record.cpp), all built by crc_init when the context is created
struct CrcTables {
    uint32_t* zpow = nullptr;                  // "append 2^j zero bytes" operators [kCrcPows][32]
    uint32_t* acc = nullptr;                   // t3hip_crc32[_dev]: [0] xor accumulator, [1] symbol sum (under acc_mu)
    uint32_t* afrag4 = nullptr;                // bit-matrix slices [14][64][4] of the FP4 CRC kernel (t3_crc_fp4.hip)
    uint32_t* afb = nullptr;                   // its feedback slices "append 2048 W zero bytes", one [64][4] per stride level
    uint32_t* dist_lo = nullptr;               // strided form, a wave's distance to the stream's end by table: "append n bytes" [2048][32] ...
    uint32_t* dist_hi = nullptr;               // ... and "append 2048 n bytes" [W0 + 1][32], W0 = the widest stride; entry 0 of both = identity
    std::mutex acc_mu;
    void release() { free_dev(zpow); free_dev(acc); free_dev(afrag4); free_dev(afb); free_dev(dist_lo); free_dev(dist_hi); }
};
// Tables of the RGB8 <-> quantised YCbCr bridge, built on first use
struct RgbTables {
    QuantTables* quant = nullptr;              // the bridge kernels' tables (t3_api_rgb.cpp, under Ctx::qt_mu)
    uint8_t* chroma_q = nullptr;               // chroma quantiser of the encoder's fused RGB front end (t3_api_encode.cpp, under Ctx::mu)
    uint8_t* dequant = nullptr;                // dequantiser of the decoder's fused RGB output stage (t3_api_decode.cpp, under Ctx::tab_mu)
    void release() { free_dev(quant); free_dev(chroma_q); free_dev(dequant); }
};
// Pinned host memory of the synchronous decode entry points (t3_api_decode.cpp, under Ctx::mail_mu)
struct Mailboxes {
    uint8_t* header = nullptr;                 // read_header's 54 / 90 header bytes
    uint32_t* fail = nullptr; uint32_t* d_fail = nullptr;   // mapped failure counter and its device address
    void release() { free_pinned(header); free_pinned(fail); d_fail = nullptr; }
};

// Grow-only device scratch.  Host* are per context (the host-buffer entry points, under Ctx::host_mu); Stream* are per (kind, caller
// stream), so that the *_dev entry points may have frames in flight on several streams (hipStreamPerThread: one per thread).
enum class Scratch {
    HostIn, HostOut,                           // upload / download buffers of the host-buffer entry points
    StreamBody,                                // a coded body without its beacons (encoder beacon pass, decoder debeacon pass)
    StreamWork,                                // decoder intermediates (UEP edge records, two-kernel symbol stream, generic decoder)
    StreamRgb,                                 // quantised pixels of the RGB bridge paths
    StreamWindow,                              // the decoded run of pixels a window is cropped from (t3hip_decode_window_async)
    StreamImage,                               // the composed RGB frame of t3hip_encode_image_dev
    StreamCrc,                                 // slots and records of t3hip_crc32_frames[_dev] (under CrcTables::acc_mu)
    StreamErasure,                             // the private copy and the work words of t3hip_decode_erasures_* (t3_api_decode_era.cpp)
    StreamEraVerdict,                          // the verdict words of t3hip_decode_erasures_frames_dev (four per frame)
};

struct Ctx {
    int dev = -1; bool ready = false; int n_cu = 256;
    hipStream_t stream = nullptr;                       // used by the host-buffer entry points
    RsTables* d_tab = nullptr;
    uint8_t* d_P[4][2] = {};                            // RS parity matrices per k index and mode
    std::map<uint32_t, LutImage> luts;                  // encoder tables; key = kmask | mode << 8 (| kind << 16)
    void* buf[2] = {}; size_t cap[2] = {};              // Scratch::HostIn, HostOut
    std::map<std::pair<Scratch, hipStream_t>, std::pair<void*, size_t>> sbuf;          // Scratch::Stream*
    uint32_t* d_ctr = nullptr; std::map<std::pair<hipStream_t, int>, uint32_t> ctr_slot;   // tile-ticket counters, one set per (stream, kernel kind) in use
    uint32_t* d_flag = nullptr;                         // failure counter for the synchronous decode entry points
    hipStream_t stream2 = nullptr;                      // the download side of the pipelined host entry points (run_chunks, created on first use)
    std::vector<hipEvent_t> chunk_ev;                   // ... and their per-chunk events
    DecodeTables dec; CrcTables crc; RgbTables rgb; Mailboxes mail;
    std::string hip_err;
    std::mutex mu;                                      // encoder tables, scratch, ticket counters
    // The host-buffer entry points share one stream and the Host* scratch: each of them holds this for its whole upload -> launch ->
    // download -> synchronise sequence (two caller threads otherwise interleave on the stream and overwrite, or free, each other's
    // scratch).  Recursive: some of them are built from others.
    std::recursive_mutex host_mu;
    std::mutex tab_mu, qt_mu;                           // lazily built tables of the decode / RGB halves (per context: contexts share no lock)
    std::mutex mail_mu;                                 // pinned mailboxes of the synchronous decode entry points
};

// The calling thread's context (t3hip_use), else the process default (t3hip_init), else a stand-in with ready == false.
Ctx& ctx();
int fail_hip(hipError_t e, const char* what);           // records the error in ctx(); returns T3_E_HIP
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return ::t3::fail_hip(e_, #x); } while (0)

// These take c.mu themselves; the *_held forms are for a caller that holds it (the encoder plans and launches a frame under it).
int scratch(Ctx& c, Scratch kind, size_t bytes, void** out, hipStream_t s = nullptr);
int scratch_held(Ctx& c, Scratch kind, size_t bytes, void** out, hipStream_t s = nullptr);
// Tile tickets of a persistent launch of `grid` workgroups on s: *ctr = the zeroed counter set of (s, kind) -- kind 0 encoder, 1 pixel
// decoder, 2 UEP decoder -- or nullptr (static tiles: T3HIP_STATIC_TILES, a measurement knob read once, hipStreamPerThread, no set left);
// *n_classes = min(8, grid).
void tile_tickets(Ctx& c, hipStream_t s, int kind, uint32_t grid, uint32_t** ctr, uint32_t* n_classes);
void tile_tickets_held(Ctx& c, hipStream_t s, int kind, uint32_t grid, uint32_t** ctr, uint32_t* n_classes);

// The persistent grid of fn: what is resident at once, at most n_items, at least one workgroup.  Workgroups per CU from the occupancy query
// (VGPR, LDS and wave limits), cached per (function, device, threads, LDS bytes) under one process-wide lock, the dynamic-LDS attribute set
// on the first query; round_lds_units: also at most as many as the LDS units above allow.
int resident_grid(Ctx& c, const void* fn, int threads, uint32_t lds_bytes, uint64_t n_items, bool round_lds_units, uint32_t* grid);
// The pipelined host entry points (the caller holds c.host_mu; t3_api.cpp).  A frame crosses PCIe in chunks of whole tiles: the caller's
// thread runs upload_and_launch(ch) on c.stream for one chunk after the other and records chunk ch's event behind it; a helper thread
// waits for that event and runs download(ch, s2) on the download stream meanwhile (pageable memory: a HIP copy occupies its calling thread,
// so the two directions need two threads).  Returns the first error, T3_OK once both streams have drained, or 1 -- nothing issued -- when
// the helper thread cannot be started (the caller takes its serial path).
int run_chunks(Ctx& c, uint32_t n_chunks, const std::function<int(uint32_t ch)>& upload_and_launch,
               const std::function<hipError_t(uint32_t ch, hipStream_t s2)>& download);
// the band runs of blocks [blk_lo, blk_hi) of every band of a band-serial stream (hs header symbols in front), src -> dst at the same
// offsets on s: one strided copy when allow_strided, the nine bands are equally long, the window lies inside them and offset, width and
// pitch are 4-byte aligned; else one copy per band
hipError_t copy_band_runs(uint8_t* dst, const uint8_t* src, const t3_layout& L, uint32_t hs, uint64_t blk_lo, uint64_t blk_hi,
                          bool allow_strided, hipMemcpyKind kind, hipStream_t s);
bool equal_band_runs(const t3_layout& L);               // the nine bands equally long, their pitch 4-byte aligned
uint32_t host_chunks(uint32_t dflt);                    // chunks per frame: the measurement knob of t3_api.cpp (read once), else dflt
// the fused RGB encode (t3_api_encode.cpp); 1: that framing is not fused, the caller takes the bridge path
int encode_rgb_fused(const void* d_rgb, uint64_t n_px, const t3_cfg* cfg, void* d_out, uint64_t cap, uint64_t* n_out, hipStream_t s);
// A batch of equal frames, planned (t3hip_frames_plan; t3_api_encode.cpp): host arithmetic only.  decode = 0 / 1; fmt: the unit side of the call
// (0 raw words, 1 pixels, 2 RGB8); n_units: units of one frame on that side.  L: one frame's layout.  T3_OK or T3_E_ARG.
int plan_frames(int decode, uint64_t n_units, uint32_t n_frames, const t3_cfg& cfg, int fmt, t3_frames_plan& out, t3_layout& L);
// strides and bases of a batch call against its plan (n_frames >= 2): 16-byte aligned, strides at least the plan's minima
inline bool frames_strides_ok(const t3_frames_plan& fp, const void* in, uint64_t in_stride, const void* out, uint64_t out_stride) {
    return (((uintptr_t)in | (uintptr_t)out | in_stride | out_stride) & 15u) == 0 && in_stride >= fp.in_stride_min && out_stride >= fp.out_stride_min;
}
// host <-> device copy of the frames of a batch on s, their own bytes only (the gaps of a stride are neither read nor written): one copy,
// strided when the frames are not back to back
inline hipError_t copy_frames(void* dst, const void* src, uint64_t stride, uint64_t bytes, uint32_t n_frames, hipMemcpyKind kind, hipStream_t s) {
    if (!n_frames || !bytes) return hipSuccess;
    if (n_frames == 1 || stride == bytes) return hipMemcpyAsync(dst, src, (uint64_t)(n_frames - 1) * stride + bytes, kind, s);
    return hipMemcpy2DAsync(dst, stride, src, stride, bytes, n_frames, kind, s);
}
int decode_init(DecodeTables& tab);                     // builds the field tables (t3_api_decode.cpp)
// The bind step of a fused FIXED launch planned by plan_fixed_fused (t3_dec_plan.hpp; t3_api_decode.cpp): tables, pointers, kernel, grid.
// n_frames > 0: a batch, the grid over the tiles of all frames; fn: the caller's kernel on the plan's arguments (the repair kernels)
struct FusedPlan;
int bind_fused(FusedPlan& p, void* d_out, uint32_t* d_fail, uint32_t n_frames = 0, const void* fn = nullptr);
// The two kinds of repair (t3_api_repair.cpp): verdict words per frame, and the kernels by k index -- one frame, a batch of frames -- and
// the generic one.  Plain: four words (t3_repair.hip, t3_repair_frames.hip); bytes above 26 as erasures: six (t3_repair_era.hip,
// t3_repair_era_frames.hip), on the same argument blocks
struct RepairKind { uint32_t nw; const void* fixed[4]; const void* frames[4]; const void* generic; };
const RepairKind& repair_erasures();                   // (the erasure decoder's path 0 repairs its private copy)
// The repair of a frame's body on `s` (t3_api_repair.cpp): verdict words zeroed, [0] by hdr_compare_kernel when hx is given, ONE launch of
// the kernel plan P names
struct HdrExpect;
int repair_body(void* d_io, const t3_cfg& cfg, const t3_layout& L, const t3_repair_plan& P, const uint8_t next[3], uint32_t flags,
                uint32_t* d_verdict, const HdrExpect* hx, uint32_t hs, hipStream_t s, const RepairKind& kind);
// The synchronous entries' two reads (t3_api.cpp), each one copy on s and s synchronised: the 90 header bytes of n_frames frames `stride`
// apart (one frame: the stride is not looked at) into got, back to back; the nw verdict words of every frame, folded into counts and
// frame_rc for the frames that ran (fold_verdicts, t3_frame_batch.hpp)
int fetch_headers(uint8_t* got, const void* d_frames, uint64_t stride, uint32_t n_frames, hipStream_t s);
int fetch_verdicts(const void* d_v, uint32_t nw, uint32_t n_frames, const uint8_t* go, uint32_t* counts, int* frame_rc, hipStream_t s);
// The streaming decoders on the body of a frame whose configuration is known, the scrambler as its next-state table, no header check
// (t3_api_decode.cpp: decode_body); fmt 2 (RGB8) where no fused kernel serves the framing: pixels into Scratch::StreamRgb, then the bridge
int decode_body_known(const void* d_in, uint64_t n_in, const t3_cfg& cfg, uint64_t n_raw, const uint8_t next[3], void* d_out, uint64_t cap_units,
                      uint64_t* n_out, int fmt, uint32_t* d_fail, hipStream_t s);
// ... and a w x h window of such a frame the way t3hip_decode_window_async takes its whole-frame path (t3_api_decode.cpp): the frame's pixels
// by decode_body_known into Scratch::StreamWindow, then window_crop_kernel into d_out (out_fmt 1 pixels, 2 RGB8; 4-byte aligned)
int decode_window_known(const void* d_in, uint64_t n_in, const t3_cfg& cfg, uint64_t n_raw, const uint8_t next[3], uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                        uint32_t w, uint32_t h, void* d_out, int out_fmt, uint32_t* d_fail, hipStream_t s);
// measurement / test knob T3HIP_GENERIC_DECODE: the generic kernels for every framing (the plans take it as a flag; every window plan asks here)
inline bool generic_decode() { return getenv("T3HIP_GENERIC_DECODE") != nullptr; }
// the instantiation of a kernel template for r = 26 - k parity symbols: pick(std::integral_constant<int, r>) names it
template <class F> const void* by_r(int r, F pick) {
    return r == 2 ? pick(std::integral_constant<int, 2>{}) : r == 4 ? pick(std::integral_constant<int, 4>{}) : r == 6 ? pick(std::integral_constant<int, 6>{}) : pick(std::integral_constant<int, 8>{});
}
int crc_init(Ctx& c);                                   // builds c.crc for c.n_cu (t3_api_record.cpp)
// Staging of the host-buffer entry points (the caller holds c.host_mu): `in` up into Scratch::HostIn, Scratch::HostOut sized for
// out_bytes (both + 64); then `bytes` of the result back and c.stream synchronised.
int host_stage(Ctx& c, const void* in, uint64_t in_bytes, void** di, uint64_t out_bytes, void** dout);
int host_fetch(Ctx& c, void* out, const void* dout, uint64_t bytes);

// The failure counter of the synchronous decode entry points in mapped pinned host memory, allocated on first use and zeroed: written only
// by lanes that give up on a block, read after the sync without a copy (the previous synchronous call has drained, so the host may clear
// it directly).  Returns its device address, nullptr after a HIP error (recorded).  The caller holds c.mail_mu.
inline uint32_t* arm_fail_mailbox(Ctx& c) {
    Mailboxes& m = c.mail; hipError_t e = hipSuccess;
    if (!m.fail) { e = hipHostMalloc((void**)&m.fail, 64, hipHostMallocMapped); if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&m.d_fail, m.fail, 0); }
    if (e != hipSuccess) { fail_hip(e, "arm_fail_mailbox"); free_pinned(m.fail); m.d_fail = nullptr; return nullptr; }
    *(volatile uint32_t*)m.fail = 0;
    return m.d_fail;
}

// workgroups of 256 threads for `items` work items: at least one, at most `cap`
inline unsigned blocks_for(uint64_t items, uint64_t cap = 1u << 30) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, (items + 255) / 256), cap); }

}  // namespace t3
