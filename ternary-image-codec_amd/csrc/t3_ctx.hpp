// t3_ctx.hpp — the library context (one per GPU, t3_api.cpp) and the helpers the host translation units share.
// Host code only: t3_api*.cpp include it, no .hip file does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/t3hip.h"

namespace t3 {

struct RsTables; struct FxTables; struct QuantTables;

template <class T> void free_dev(T*& p) { if (p) (void)hipFree((void*)p); p = nullptr; }
template <class T> void free_pinned(T*& p) { if (p) (void)hipHostFree((void*)p); p = nullptr; }

struct LutImage { uint32_t* d_img = nullptr; uint32_t bytes = 0; uint32_t k_off[4] = {0, 0, 0, 0}; uint32_t* d_afrag = nullptr; };

// Device tables of the decode half (t3_api_decode.cpp): the CRC operators and field tables decode_init builds, then the tables of
// one code, built on first use under Ctx::tab_mu.  Arrays [4] are indexed by k index (k = 24, 22, 20, 18).
struct DecodeTables {
    uint32_t* zpow = nullptr;                  // CRC "append 2^j zero bytes" operators
    uint32_t* crc_acc = nullptr;               // [0] xor accumulator, [1] symbol sum (under Ctx::mail_mu)
    uint32_t* crc_afrag = nullptr;             // bit-matrix slices of the matrix-core CRC (t3_crc_mfma.hip) ...
    uint32_t* crc_afrag4 = nullptr;            // ... of its FP4 form (t3_crc_fp4.hip)
    uint32_t* crc_afb = nullptr; uint32_t crc_afb_w = 0;   // FP4 CRC, strided rounds: the feedback slices "append 2048 W zero bytes", and W
    FxTables* fxtab = nullptr;                 // field tables of the two-kernel FIXED decoder
    uint8_t* fma = nullptr;                    // fma[x][y][a] = a + x y: one table read per multiply-accumulate of the corrector
    uint32_t* synd_T = nullptr; uint32_t* synd_T16 = nullptr;   // descramble + trit expansion table of the syndrome MFMA, 32 / 16 bank copies
    uint8_t* fx2_small = nullptr;              // log / exp / inverse byte tables + fold tables of the fused decoders
    uint32_t* synd_lut[4] = {}; uint32_t synd_lut_bytes[4] = {};   // syndrome LUT of the two-kernel decoder
    uint32_t* roots[4] = {};                   // the Chien search (OLD:611-623) of every locator, tabulated
    uint32_t* synd_afrag[4] = {};              // A operand of the syndrome MFMA (t3_host.hpp build_mfma_syndrome)
    void release() {
        free_dev(zpow); free_dev(crc_acc); free_dev(crc_afrag); free_dev(crc_afrag4); free_dev(crc_afb); crc_afb_w = 0;
        free_dev(fxtab); free_dev(fma); free_dev(synd_T); free_dev(synd_T16); free_dev(fx2_small);
        for (int i = 0; i < 4; ++i) { free_dev(synd_lut[i]); synd_lut_bytes[i] = 0; free_dev(roots[i]); free_dev(synd_afrag[i]); }
    }
};
// Tables of the RGB8 <-> quantised YCbCr bridge, built on first use
struct RgbTables {
    QuantTables* quant = nullptr;              // the bridge kernels' tables (t3_api_rgb.cpp, under Ctx::qt_mu)
    uint8_t* chroma_q = nullptr;               // chroma quantiser of the encoder's fused RGB front end (t3_api.cpp, under Ctx::mu)
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
    hipStream_t stream2 = nullptr;                      // the download side of the pipelined host entry points (created on first use)
    std::vector<hipEvent_t> chunk_ev;                   // ... and their per-chunk events
    DecodeTables dec; RgbTables rgb; Mailboxes mail;
    std::string hip_err;
    std::mutex mu;                                      // encoder tables, scratch, ticket counters
    // The host-buffer entry points share one stream and the Host* scratch: each of them holds this for its whole upload -> launch ->
    // download -> synchronise sequence (two caller threads otherwise interleave on the stream and overwrite, or free, each other's
    // scratch).  Recursive: some of them are built from others.
    std::recursive_mutex host_mu;
    std::mutex tab_mu, qt_mu;                           // lazily built tables of the decode / RGB halves (per context: contexts share no lock)
    std::recursive_mutex mail_mu;                       // pinned mailboxes + CRC accumulator of the synchronous entry points
};

// The calling thread's context (t3hip_use), else the process default (t3hip_init), else a stand-in with ready == false.
Ctx& ctx();
int fail_hip(hipError_t e, const char* what);           // records the error in ctx(); returns T3_E_HIP
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return ::t3::fail_hip(e_, #x); } while (0)

// These take c.mu themselves.
int scratch(Ctx& c, Scratch kind, size_t bytes, void** out, hipStream_t s = nullptr);
uint32_t* ticket_counters(Ctx& c, hipStream_t s, int kind);         // kind: 0 encoder, 1 pixel decoder, 2 UEP decoder; nullptr: static tiles
// the download stream and per-chunk events of the pipelined host entry points (the caller holds c.host_mu)
int pipeline(Ctx& c, uint32_t n_events, hipStream_t* s2, hipEvent_t** evs);
// the fused RGB encode (t3_api.cpp); 1: that framing is not fused, the caller takes the bridge path
int encode_rgb_fused(const void* d_rgb, uint64_t n_px, const t3_cfg* cfg, void* d_out, uint64_t cap, uint64_t* n_out, hipStream_t s);
int decode_init(DecodeTables& tab);                     // builds the CRC operators and field tables (t3_api_decode.cpp)
// Staging of the host-buffer entry points (the caller holds c.host_mu): `in` up into Scratch::HostIn, Scratch::HostOut sized for
// out_bytes (both + 64); then `bytes` of the result back and c.stream synchronised.
int host_stage(Ctx& c, const void* in, uint64_t in_bytes, void** di, uint64_t out_bytes, void** dout);
int host_fetch(Ctx& c, void* out, const void* dout, uint64_t bytes);

}  // namespace t3
