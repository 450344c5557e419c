// t3_api.cpp — what every host unit of libt3hip.so shares (t3_ctx.hpp): the context and its life cycle, the scratch, ticket and occupancy
// caches, the chunk pipeline of the host-buffer entry points; and of the C-ABI (include/t3hip.h) the status functions, the host-only
// metadata and the timing events.  The encode half: t3_api_encode.cpp; the decode half: t3_api_decode.cpp.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_frame_batch.hpp"
#include "t3_host.hpp"

using namespace t3;

namespace {

// One context per GPU.  t3hip_init creates the process default; t3hip_create more (one per device for a host that drives a whole
// node from one process); t3hip_use binds the calling thread to one of them (thread-local), every entry point works on the
// calling thread's context: ctx().
Ctx g_null;                                               // stands in while no context exists: ready == false
Ctx* g_def = nullptr;
thread_local Ctx* tl_cur = nullptr;

int grow(void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return T3_OK;
    if (p) HIPCHK(hipFree(p));                           // synchronises with whatever still reads it
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 8 + 4096;
    HIPCHK(hipMalloc(&p, want));
    cap = want;
    return T3_OK;
}
}  // namespace

Ctx& t3::ctx() { return tl_cur ? *tl_cur : (g_def ? *g_def : g_null); }
int t3::fail_hip(hipError_t e, const char* what) { ctx().hip_err = std::string(what) + ": " + hipGetErrorString(e); return T3_E_HIP; }

// Tile-ticket counters of a persistent kernel (tile_tickets, t3_ctx.hpp): eight class counters + a done counter, 256 B apart, zero between
// launches (the kernel's last workgroup re-zeroes them).  One set per (stream, kernel kind): launches on one stream are ordered, streams are
// not.  None for hipStreamPerThread (one handle value, a different real stream per thread) or when the allocation failed.
void t3::tile_tickets_held(Ctx& c, hipStream_t s, int kind, uint32_t grid, uint32_t** ctr, uint32_t* n_classes) {
    constexpr uint32_t kSlots = 64, kSlotWords = 64 * 9;
    static const bool off = getenv("T3HIP_STATIC_TILES") != nullptr;      // measurement knob
    *n_classes = std::min<uint32_t>(8u, grid); *ctr = nullptr;
    if (off || s == hipStreamPerThread) return;
    if (!c.d_ctr) { if (hipMalloc((void**)&c.d_ctr, kSlots * kSlotWords * 4) != hipSuccess) { c.d_ctr = nullptr; return; } if (hipMemset(c.d_ctr, 0, kSlots * kSlotWords * 4) != hipSuccess) return; }
    const auto key = std::make_pair(s, kind);
    auto sl = c.ctr_slot.find(key);
    if (sl == c.ctr_slot.end() && c.ctr_slot.size() < kSlots) sl = c.ctr_slot.emplace(key, (uint32_t)c.ctr_slot.size()).first;
    if (sl != c.ctr_slot.end()) *ctr = c.d_ctr + kSlotWords * sl->second;
}

int t3::scratch_held(Ctx& c, Scratch kind, size_t bytes, void** out, hipStream_t s) {
    if (kind == Scratch::HostIn || kind == Scratch::HostOut) {
        const int i = kind == Scratch::HostIn ? 0 : 1;
        const int rc = grow(c.buf[i], c.cap[i], bytes); if (rc) return rc;
        *out = c.buf[i];
        return T3_OK;
    }
    static thread_local char per_thread_key;              // hipStreamPerThread is one handle value but a different stream in every thread
    if (s == hipStreamPerThread) s = (hipStream_t)(void*)&per_thread_key;
    auto& e = c.sbuf[std::make_pair(kind, s)];
    const int rc = grow(e.first, e.second, bytes); if (rc) return rc;
    *out = e.first;
    return T3_OK;
}

extern "C" {

int t3hip_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

static int ctx_init_in(Ctx* c, int device);
static void ctx_teardown(Ctx* c);
// Builds `c` on `device`.  The calling thread's current context is `c` for the whole of it, so a HIP error (HIPCHK) is recorded in `c` (and
// copied to the null context for t3hip_last_hip_error after a failed create); what a failed build had already allocated is released.
static int ctx_init(Ctx* c, int device) {
    Ctx* const prev = tl_cur; tl_cur = c;
    const int rc = ctx_init_in(c, device);
    tl_cur = prev;
    if (rc) { const std::string err = c->hip_err; ctx_teardown(c); g_null.hip_err = err; c->hip_err = err; }
    return rc;
}
static int ctx_init_in(Ctx* c, int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return T3_E_NODEVICE;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t p; HIPCHK(hipGetDeviceProperties(&p, device));
    if (std::string(p.gcnArchName).find("gfx950") == std::string::npos) { c->hip_err = std::string("not a gfx950 device: ") + p.gcnArchName; return T3_E_NODEVICE; }
    c->n_cu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const Field& F = field();
    HIPCHK(hipMalloc((void**)&c->d_tab, sizeof(RsTables)));
    HIPCHK(hipMemcpy(c->d_tab, &F.t, sizeof(RsTables), hipMemcpyHostToDevice));
    for (int i = 0; i < 4; ++i) for (int m = 0; m < 2; ++m) {
        uint8_t P[24 * 8]; rs_parity_matrix(kOfIndex[i], m, P);
        HIPCHK(hipMalloc((void**)&c->d_P[i][m], sizeof P));
        HIPCHK(hipMemcpy(c->d_P[i][m], P, sizeof P, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc((void**)&c->d_flag, 64));
    c->dev = device;
    int rc = decode_init(c->dec);
    if (!rc) rc = crc_init(*c);
    if (rc) return rc;
    c->ready = true;
    return T3_OK;
}
// Frees everything `c` holds, also of a partly built context (ctx_init failed): every member is null-safe.  No other thread uses `c` by
// then.  The calling thread's current context is left alone, unless it is `c`.
static void ctx_teardown(Ctx* c) {
    if (c->dev >= 0) { (void)hipSetDevice(c->dev); (void)hipDeviceSynchronize(); }
    for (auto& kv : c->luts) { free_dev(kv.second.d_img); free_dev(kv.second.d_afrag); }
    c->luts.clear();
    for (auto& kv : c->sbuf) free_dev(kv.second.first);
    c->sbuf.clear();
    for (int i = 0; i < 2; ++i) { free_dev(c->buf[i]); c->cap[i] = 0; }
    for (auto& P : c->d_P) for (uint8_t*& p : P) free_dev(p);
    c->dec.release(); c->crc.release(); c->rgb.release(); c->mail.release();
    free_dev(c->d_ctr); c->ctr_slot.clear();
    for (hipEvent_t e : c->chunk_ev) (void)hipEventDestroy(e);
    c->chunk_ev.clear();
    if (c->stream2) { (void)hipStreamDestroy(c->stream2); c->stream2 = nullptr; }
    free_dev(c->d_tab); free_dev(c->d_flag);
    if (c->stream) { (void)hipStreamDestroy(c->stream); c->stream = nullptr; }
    c->ready = false; c->dev = -1;
    if (tl_cur == c) tl_cur = nullptr;
}
static std::mutex g_ctx_mu;

int t3hip_init(int device) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (g_def && g_def->ready) return g_def->dev == device ? T3_OK : T3_E_ARG;      // the default context stays on its device: t3hip_shutdown first, or t3hip_create
    if (!g_def) g_def = new Ctx();
    const int rc = ctx_init(g_def, device);
    if (rc) { delete g_def; g_def = nullptr; }
    return rc;
}

int t3hip_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (!g_def) return T3_OK;
    if (g_def->ready) ctx_teardown(g_def);
    if (tl_cur == g_def) tl_cur = nullptr;
    delete g_def; g_def = nullptr;
    return T3_OK;
}

int t3hip_create(int device, t3hip_ctx** out) {
    if (!out) return T3_E_ARG;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    int prev_dev = -1; (void)hipGetDevice(&prev_dev);
    Ctx* c = new Ctx();
    const int rc = ctx_init(c, device);
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    if (rc) { delete c; return rc; }
    *out = (t3hip_ctx*)c;
    return T3_OK;
}
int t3hip_destroy(t3hip_ctx* h) {
    if (!h) return T3_OK;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    Ctx* c = (Ctx*)h;
    if (c == g_def) return T3_E_ARG;                      // the default context goes with t3hip_shutdown
    int prev_dev = -1; (void)hipGetDevice(&prev_dev);
    if (c->ready) ctx_teardown(c);
    if (tl_cur == c) tl_cur = nullptr;
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    delete c;
    return T3_OK;
}
int t3hip_use(t3hip_ctx* h) {
    Ctx* c = (Ctx*)h;
    if (c && !c->ready) return T3_E_ARG;
    tl_cur = c;
    Ctx& eff = ctx();                                     // c, or the default context when c is null
    if (eff.ready) HIPCHK(hipSetDevice(eff.dev));
    return T3_OK;
}
t3hip_ctx* t3hip_current(void) { Ctx& c = ctx(); return c.ready ? (t3hip_ctx*)&c : nullptr; }
int t3hip_ctx_device(const t3hip_ctx* h) { const Ctx* c = h ? (const Ctx*)h : &ctx(); return c->ready ? c->dev : -1; }
int t3hip_is_ready(void) { return ctx().ready ? 1 : 0; }
const char* t3hip_strerror(int c) {
    switch (c) {
        case T3_OK: return "ok"; case T3_E_NODEVICE: return "no usable gfx950 device (t3hip_init not done or failed)";
        case T3_E_HIP: return "HIP runtime error"; case T3_E_ARG: return "bad argument"; case T3_E_CAPACITY: return "output buffer too small";
        case T3_E_HEADER: return "superframe header did not decode (RS/CRC-12)"; case T3_E_RS: return "uncorrectable RS block";
        case T3_E_COMM: return "RCCL unavailable or collective failed";
    }
    return "unknown";
}
const char* t3hip_last_hip_error(void) { return ctx().hip_err.c_str(); }
const char* t3hip_version(void) { return "t3hip 0.1 (gfx950)"; }

// ---- host-only metadata ---------------------------------------------------------------------------------
void t3hip_cfg_default(t3_cfg* c) {
    memset(c, 0, sizeof *c);
    c->profile = T3_P2_RS26_22; for (int b = 0; b < 9; ++b) c->band_profile[b] = 1;     // OLD:864,898
    c->seed_a = c->seed_b = c->seed_s0 = 1; c->superframe_words = 8192; c->subword = 27; c->centered = 1;
}
int t3hip_plan(uint64_t n_raw, const t3_cfg* cfg, t3_layout* out) { if (!cfg || !out) return T3_E_ARG; return plan(n_raw, *cfg, *out); }
uint64_t t3hip_encoded_words(uint64_t n_raw, const t3_cfg* cfg) { t3_layout L; if (!cfg || plan(n_raw, *cfg, L) != T3_OK) return 0; return L.out_words; }
int t3hip_gf27_tables(uint8_t* e78, int16_t* l27, uint8_t* m729, uint8_t* i27) {
    const Field& F = field();
    if (e78) memcpy(e78, F.exp78, 78); if (l27) memcpy(l27, F.log, sizeof F.log);
    if (m729) memcpy(m729, F.t.mul, 729); if (i27) memcpy(i27, F.t.inv, 27);
    return T3_OK;
}
int t3hip_rs_generator(int k, uint8_t* g_out) { if (!valid_k(k) || !g_out) return T3_E_ARG; rs_generator(k, g_out); return T3_OK; }
int t3hip_mfma_encode_tables(int k, int mode, uint32_t* afrag, uint32_t* lds_img) {
    if (!valid_k(k) || !afrag || !lds_img || mode < 0 || mode > 1) return T3_E_ARG;
    std::vector<uint32_t> a, l; build_mfma_encode(k, mode, a, l);
    memcpy(afrag, a.data(), a.size() * 4); memcpy(lds_img, l.data(), l.size() * 4);
    return T3_OK;
}
int t3hip_rs_parity_matrix(int k, int mode, uint8_t* P) { if (!valid_k(k) || !P || mode < 0 || mode > 1) return T3_E_ARG; rs_parity_matrix(k, mode, P); return T3_OK; }
int t3hip_header_pack(const t3_cfg* c, uint32_t fs, uint32_t bh, uint8_t s[27]) { if (!c || !s) return T3_E_ARG; header_pack(*c, fs, bh, s); return T3_OK; }
int t3hip_header_check(const uint8_t s[27]) { return s && header_check(s) ? 1 : 0; }
int t3hip_header_unpack(const uint8_t s[27], t3_cfg* o, uint32_t* fs, uint32_t* bh) { if (!s || !o) return T3_E_ARG; header_unpack(s, *o, fs, bh); return T3_OK; }
int t3hip_header_encode(const t3_cfg* c, uint64_t n_raw, uint8_t* out, uint32_t* n) {
    if (!c || !out || !n) return T3_E_ARG;
    t3_layout L; int rc = plan(n_raw, *c, L); if (rc) return rc;
    if (c->profile == T3_RAW_MODE) { *n = 0; return T3_OK; }
    *n = (uint32_t)header_encode(*c, n_raw, out); return T3_OK;
}

// ---- timing helper ------------------------------------------------------------------------------------------
// Timing only: a plain hipEventCreate event ends every record in a system-scope release (cache write-back and invalidate, ~4 us of
// stream time, and the kernel behind it starts cold).  These events order nothing and publish nothing, so they are created without
// that fence (profiles/launch_fixed_costs/notes.md).  T3_EVENT_FLAGS: measurement builds only.
#ifndef T3_EVENT_FLAGS
#define T3_EVENT_FLAGS hipEventDisableSystemFence
#endif
int t3hip_event_create(void** ev) { if (!ctx().ready) return T3_E_NODEVICE; hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, T3_EVENT_FLAGS)); *ev = e; return T3_OK; }
int t3hip_event_record(void* ev, void* stream) { HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return T3_OK; }
int t3hip_event_elapsed_ms(void* a, void* b, float* ms) { HIPCHK(hipEventSynchronize((hipEvent_t)b)); HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b)); return T3_OK; }
int t3hip_event_destroy(void* ev) { HIPCHK(hipEventDestroy((hipEvent_t)ev)); return T3_OK; }

}  // extern "C"

// shared with the other host translation units (t3_ctx.hpp)
namespace t3 {
int scratch(Ctx& c, Scratch kind, size_t bytes, void** out, hipStream_t s) { std::lock_guard<std::mutex> lk(c.mu); return scratch_held(c, kind, bytes, out, s); }
void tile_tickets(Ctx& c, hipStream_t s, int kind, uint32_t grid, uint32_t** ctr, uint32_t* n_classes) { std::lock_guard<std::mutex> lk(c.mu); tile_tickets_held(c, s, kind, grid, ctr, n_classes); }
int resident_grid(Ctx& c, const void* fn, int threads, uint32_t lds_bytes, uint64_t n_items, bool round_lds_units, uint32_t* grid) {
    static std::map<std::tuple<const void*, int, int, uint32_t>, int> occ; static std::mutex occ_mu;   // per device: the attribute is set on the device's copy of the function
    int per_cu;
    {
        std::lock_guard<std::mutex> lk(occ_mu);
        const auto key = std::make_tuple(fn, c.dev, threads, lds_bytes);
        auto it = occ.find(key);
        if (it == occ.end()) {
            HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            int o = 1; HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, fn, threads, lds_bytes));
            it = occ.emplace(key, o).first;
        }
        per_cu = it->second;
    }
    if (round_lds_units) per_cu = std::min<int>(per_cu, (int)(kLdsUnitsPerCu / ((lds_bytes + kLdsUnit - 1u) / kLdsUnit)));
    *grid = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_items, (uint64_t)c.n_cu * (uint64_t)std::max(1, per_cu)));
    return T3_OK;
}
bool equal_band_runs(const t3_layout& L) {                // the nine bands equally long, their pitch 4-byte aligned (copy_band_runs)
    for (int b = 1; b < 9; ++b) if (L.band_blocks[b] != L.band_blocks[0]) return false;
    return (26 * L.band_blocks[0]) % 4u == 0;
}
hipError_t copy_band_runs(uint8_t* dst, const uint8_t* src, const t3_layout& L, uint32_t hs, uint64_t blk_lo, uint64_t blk_hi,
                          bool allow_strided, hipMemcpyKind kind, hipStream_t s) {
    // every copy costs ~20 us of the issuing thread; a strided copy at 2-byte alignment falls off a cliff (measured: t3_api_encode.cpp, the pipelined host entry)
    const uint64_t off = hs + L.band_body_off[0] + 26 * blk_lo, width = 26 * (blk_hi - blk_lo), pitch = 26 * L.band_blocks[0];
    if (allow_strided && equal_band_runs(L) && blk_hi <= L.band_blocks[0] && off % 4u == 0 && width % 4u == 0)
        return hipMemcpy2DAsync(dst + off, pitch, src + off, pitch, width, 9, kind, s);
    for (int b = 0; b < 9; ++b) {
        const uint64_t lo = std::min<uint64_t>(L.band_blocks[b], blk_lo), hi = std::min<uint64_t>(L.band_blocks[b], blk_hi), o = hs + L.band_body_off[b] + 26 * lo;
        if (hi > lo) { const hipError_t er = hipMemcpyAsync(dst + o, src + o, 26 * (hi - lo), kind, s); if (er != hipSuccess) return er; }
    }
    return hipSuccess;
}
uint32_t host_chunks(uint32_t dflt) { static const uint32_t env = getenv("T3HIP_HOST_CHUNKS") ? (uint32_t)atoi(getenv("T3HIP_HOST_CHUNKS")) : 0u; return env ? env : dflt; }
int run_chunks(Ctx& c, uint32_t n_chunks, const std::function<int(uint32_t ch)>& upload_and_launch,
               const std::function<hipError_t(uint32_t ch, hipStream_t s2)>& download) {
    if (!c.stream2) HIPCHK(hipStreamCreateWithFlags(&c.stream2, hipStreamNonBlocking));
    while (c.chunk_ev.size() < n_chunks) { hipEvent_t ev; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); c.chunk_ev.push_back(ev); }
    const hipStream_t s2 = c.stream2; const hipEvent_t* const evs = c.chunk_ev.data(); const int dev = c.dev;
    std::atomic<uint32_t> launched{0}; std::atomic<int> abort_dl{0};
    hipError_t dl_err = hipSuccess; int rc = T3_OK;
    try {
        std::thread dl([&] {                                // chunk ch's download, once its event has fired
            if (hipSetDevice(dev) != hipSuccess) { dl_err = hipErrorInvalidDevice; return; }
            for (uint32_t ch = 0; ch < n_chunks; ++ch) {
                while (launched.load(std::memory_order_acquire) <= ch) { if (abort_dl.load()) return; std::this_thread::yield(); }
                hipError_t er = hipEventSynchronize(evs[ch]);
                if (er == hipSuccess) er = download(ch, s2);
                if (er != hipSuccess) { dl_err = er; return; }
            }
            dl_err = hipStreamSynchronize(s2);
        });
        for (uint32_t ch = 0; ch < n_chunks && rc == T3_OK; ++ch) {
            rc = upload_and_launch(ch);
            if (rc == T3_OK) { const hipError_t er = hipEventRecord(evs[ch], c.stream); if (er != hipSuccess) rc = fail_hip(er, "hipEventRecord"); }
            if (rc == T3_OK) launched.store(ch + 1, std::memory_order_release);
        }
        if (rc != T3_OK) abort_dl.store(1);
        dl.join();
    } catch (const std::system_error&) {                    // only from the thread's constructor (past it, unwinding would meet a joinable
        return 1;                                           // thread and terminate): nothing issued yet
    }
    if (rc == T3_OK && dl_err != hipSuccess) rc = fail_hip(dl_err, "run_chunks: chunk download");
    if (rc == T3_OK) HIPCHK(hipStreamSynchronize(c.stream));
    else { (void)hipStreamSynchronize(s2); (void)hipStreamSynchronize(c.stream); }   // nothing left in flight into the caller's buffers
    return rc;
}
int host_stage(Ctx& c, const void* in, uint64_t in_bytes, void** di, uint64_t out_bytes, void** dout) {
    int rc = scratch(c, Scratch::HostIn, in_bytes + 64, di); if (rc) return rc;
    rc = scratch(c, Scratch::HostOut, out_bytes + 64, dout); if (rc) return rc;
    if (in_bytes) HIPCHK(hipMemcpyAsync(*di, in, in_bytes, hipMemcpyHostToDevice, c.stream));
    return T3_OK;
}
int host_fetch(Ctx& c, void* out, const void* dout, uint64_t bytes) {
    if (bytes) HIPCHK(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream)); return T3_OK;
}
int fetch_headers(uint8_t* got, const void* d_frames, uint64_t stride, uint32_t n_frames, hipStream_t s) {
    HIPCHK(hipMemcpy2DAsync(got, 90, d_frames, n_frames > 1 ? stride : 90, 90, n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s)); return T3_OK;
}
int fetch_verdicts(const void* d_v, uint32_t nw, uint32_t n_frames, const uint8_t* go, uint32_t* counts, int* frame_rc, hipStream_t s) {
    std::vector<uint32_t> v((uint64_t)nw * n_frames);
    HIPCHK(hipMemcpyAsync(v.data(), d_v, 4ull * nw * n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    fold_verdicts(v.data(), nw, n_frames, go, counts, frame_rc);
    return T3_OK;
}
}  // namespace t3
