// t3_api_rgb.cpp — C-ABI of SURVEY §8 row f1 (RGB8 <-> quantised YCbCr bridge, old/include/io_image.hpp:47-90,156-195)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_rgb.h"

using namespace t3;

namespace {
int tables(const QuantTables** out) {
    Ctx& c = ctx();
    std::lock_guard<std::mutex> lk(c.qt_mu);
    QuantTables*& d_qt = c.rgb.quant;
    if (!d_qt) {
        QuantTables t; memset(&t, 0, sizeof t);
        auto cl = [](long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); };
        for (int Y = 0; Y < 256; ++Y) t.yq[Y] = (uint16_t)cl(lround(Y * (242.0 / 255.0)), 0, 242);                  // io_image.hpp:72
        for (int C = 0; C < 256; ++C) t.cq[C] = (int8_t)cl(lround((C - 128) * (40.0 / 128.0)), -40, 40);           // :73-76
        for (int q = 0; q <= 242; ++q) t.yd[q] = (uint8_t)cl(lround(q * (255.0 / 242.0)), 0, 255);                  // :81
        for (int q = -40; q <= 40; ++q) t.cd[q + 40] = (uint8_t)cl(lround(128 + q * (128.0 / 40.0)), 0, 255);       // :82-83
        HIPCHK(hipMalloc((void**)&d_qt, sizeof t)); HIPCHK(hipMemcpy(d_qt, &t, sizeof t, hipMemcpyHostToDevice));
    }
    *out = d_qt; return T3_OK;
}
}  // namespace

extern "C" {

int t3hip_rgb_to_quant_dev(const uint8_t* d_rgb, uint64_t n_px, void* d_px6, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!n_px) return T3_OK;
    if (!d_rgb || !d_px6) return T3_E_ARG;
    const QuantTables* t; int rc = tables(&t); if (rc) return rc;
    hipLaunchKernelGGL(rgb_to_quant_kernel, dim3(blocks_for((n_px + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_rgb, n_px, (uint16_t*)d_px6, t);
    HIPCHK(hipGetLastError()); return T3_OK;
}
int t3hip_quant_to_rgb_dev(const void* d_px6, uint64_t n_px, uint8_t* d_rgb, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!n_px) return T3_OK;
    if (!d_rgb || !d_px6) return T3_E_ARG;
    const QuantTables* t; int rc = tables(&t); if (rc) return rc;
    hipLaunchKernelGGL(quant_to_rgb_kernel, dim3(blocks_for((n_px + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)d_px6, n_px, d_rgb, t);
    HIPCHK(hipGetLastError()); return T3_OK;
}
// Scratch::StreamRgb holds the quantised pixels between the two launches
int t3hip_encode_rgb_dev(const uint8_t* d_rgb, uint64_t n_px, const t3_cfg* cfg, void* d_out, uint64_t cap_words, uint64_t* n_out, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!cfg || !n_out || (n_px && !d_rgb)) return T3_E_ARG;
    // one launch: the bridge runs inside the encoder's phase 1 (3 bytes per pixel read, no intermediate); the framings that
    // kernel does not take (RAW mode, 2-D rows wider than 512) go through the bridge kernel and a per-stream scratch
    int rc = encode_rgb_fused(d_rgb, n_px, cfg, d_out, cap_words, n_out, (hipStream_t)stream);
    if (rc != 1) return rc;
    void* d_q; rc = scratch(ctx(), Scratch::StreamRgb, 6 * n_px + 64, &d_q, (hipStream_t)stream); if (rc) return rc;
    rc = t3hip_rgb_to_quant_dev(d_rgb, n_px, d_q, stream); if (rc) return rc;
    return t3hip_encode_frame_dev(d_q, n_px, cfg, d_out, cap_words, n_out, stream);
}
int t3hip_decode_rgb_async(const void* d_in, uint64_t n_in, const t3_cfg* cfg, uint64_t n_px, uint8_t* d_rgb, uint32_t* d_verdict, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!cfg || !d_verdict || (n_px && !d_rgb)) return T3_E_ARG;
    const uint64_t n_raw = (n_px + 1) / 2;
    uint64_t n_units = 0;
    // one launch where the fused pixel decoder applies (FIXED, one k, 1-D): its output stage converts to RGB and stores 3 bytes per pixel;
    // 1: it does not, and nothing has been launched -- the pixel decode (with the one header check) and the bridge kernel
    int rc = t3hip_decode_frame_async(d_in, n_in, cfg, n_raw, d_rgb, n_px, &n_units, 2, d_verdict, stream);
    if (rc != 1) return rc;
    void* d_q; rc = scratch(ctx(), Scratch::StreamRgb, 12 * n_raw + 64, &d_q, (hipStream_t)stream); if (rc) return rc;
    rc = t3hip_decode_frame_async(d_in, n_in, cfg, n_raw, d_q, 2 * n_raw, &n_units, 1, d_verdict, stream); if (rc) return rc;
    return t3hip_quant_to_rgb_dev(d_q, n_px, d_rgb, stream);
}
int t3hip_rgb_to_quant(const uint8_t* rgb, uint64_t n_px, void* px6) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_px) return T3_OK;
    if (!rgb || !px6) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout; int rc = host_stage(c, rgb, 3 * n_px, &di, 6 * n_px, &dout); if (rc) return rc;
    rc = t3hip_rgb_to_quant_dev((const uint8_t*)di, n_px, dout, c.stream); if (rc) return rc;
    return host_fetch(c, px6, dout, 6 * n_px);
}
int t3hip_quant_to_rgb(const void* px6, uint64_t n_px, uint8_t* rgb) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_px) return T3_OK;
    if (!rgb || !px6) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout; int rc = host_stage(c, px6, 6 * n_px, &di, 3 * n_px, &dout); if (rc) return rc;
    rc = t3hip_quant_to_rgb_dev(di, n_px, (uint8_t*)dout, c.stream); if (rc) return rc;
    return host_fetch(c, rgb, dout, 3 * n_px);
}

}  // extern "C"
