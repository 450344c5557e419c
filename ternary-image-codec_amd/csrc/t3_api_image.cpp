// t3_api_image.cpp — C-ABI of the image front end (old/include/io_image.hpp:102-140 resize_rgb_nn / blit_center_rgb,
// :237-337 image_to_words_subword / words_to_image_subword): geometry on the host, resize + centring blit as one kernel
// (image_compose_kernel, t3_window.hip), and the two flows composed from it, the RGB encode and the window decode.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_window.h"

using namespace t3;

namespace {
struct Geo { int fw, fh, x0, y0, tw, th; };
int geometry(int sub, int centered, Geo& g) {
    switch (sub) {                                                     // std_res_for OLD:123-136
        case 27: g.tw = 7680; g.th = 4320; break;
        case 24: g.tw = 3840; g.th = 2160; break;
        case 21: g.tw = 1920; g.th = 1080; break;
        case 18: g.tw = 1280; g.th = 720; break;
        case 15: g.tw = 854; g.th = 480; break;
        default: return T3_E_ARG;
    }
    if (centered && sub != 27) { g.fw = 7680; g.fh = 4320; g.x0 = (g.fw - g.tw) / 2; g.y0 = (g.fh - g.th) / 2; }   // centered_window OLD:141-146
    else { g.fw = g.tw; g.fh = g.th; g.x0 = g.y0 = 0; }
    return T3_OK;
}
// the sw x sh source mapped onto the tw x th window at (x0, y0) of a zeroed fw x fh frame
int launch_compose(const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int fw, int fh, int x0, int y0, int tw, int th, hipStream_t s) {
    if (fw < 0 || fh < 0) return T3_E_ARG;
    const uint64_t dst_bytes = 3ull * (uint64_t)fw * (uint64_t)fh;
    if (!dst_bytes) return T3_OK;
    if (sw >= 65536 || sh >= 65536 || fw >= 65536 || fh >= 65536) return T3_E_ARG;
    if (!d_dst || ((uintptr_t)d_dst & 3u)) return T3_E_ARG;
    if (sw <= 0 || sh <= 0) { HIPCHK(hipMemsetAsync(d_dst, 0, dst_bytes, s)); return T3_OK; }     // io_image.hpp:108: the zeroed destination
    if (!d_src) return T3_E_ARG;
    ComposeArgs a; memset(&a, 0, sizeof a);
    a.src = d_src; a.dst = d_dst; a.dst_bytes = dst_bytes;
    a.lead = (uint32_t)((uintptr_t)d_dst & 15u); a.n_gran = (a.lead + dst_bytes + 15u) / 16u;
    a.sw = (uint32_t)sw; a.sh = (uint32_t)sh; a.fw = (uint32_t)fw; a.fh = (uint32_t)fh;
    a.x0 = (uint32_t)x0; a.y0 = (uint32_t)y0; a.tw = (uint32_t)tw; a.th = (uint32_t)th;
    a.resize = (sw != tw || sh != th) ? 1u : 0u;
    // the multiply-shift division is exact below 2^31: frame bytes, and the resize map's (2 t + 1) * side
    a.wide = (dst_bytes >= (1ull << 31) || 2ull * a.tw * a.sw >= (1ull << 31) || 2ull * a.th * a.sh >= (1ull << 31)) ? 1u : 0u;
    a.div_row = to_dev(fastdiv(3u * a.fw)); a.div_fw = to_dev(fastdiv(a.fw)); a.div_tw2 = to_dev(fastdiv(2u * a.tw)); a.div_th2 = to_dev(fastdiv(2u * a.th));
    void* args[] = {(void*)&a};
    HIPCHK(hipLaunchKernel((const void*)image_compose_kernel, dim3((unsigned)((a.n_gran + 255u) / 256u)), dim3(256), args, 0, s));
    return T3_OK;
}
// n_frames sources of one size, source f at d_src + f * src_stride (any alignment), composed in one launch into frames at d_dst + f * dst_stride
// (16-byte aligned, the stride a multiple of 16); every frame is written once
int launch_compose_frames(const uint8_t* d_src, int sw, int sh, uint64_t src_stride, uint32_t n_frames, uint8_t* d_dst, uint64_t dst_stride, const Geo& g, hipStream_t s) {
    const uint64_t dst_bytes = 3ull * (uint64_t)g.fw * (uint64_t)g.fh;
    if (!dst_bytes || !n_frames) return T3_OK;
    if (sw >= 65536 || sh >= 65536 || n_frames > 65535u) return T3_E_ARG;
    if (!d_dst || (((uintptr_t)d_dst | dst_stride) & 15u) || dst_stride < dst_bytes) return T3_E_ARG;
    if (sw <= 0 || sh <= 0) { HIPCHK(hipMemsetAsync(d_dst, 0, (uint64_t)(n_frames - 1) * dst_stride + dst_bytes, s)); return T3_OK; }   // io_image.hpp:108: the zeroed destination
    if (!d_src) return T3_E_ARG;
    ComposeFramesArgs fa; memset(&fa, 0, sizeof fa);
    ComposeArgs& a = fa.a;
    a.src = d_src; a.dst = d_dst; a.dst_bytes = dst_bytes;
    a.lead = 0; a.n_gran = (dst_bytes + 15u) / 16u;
    a.sw = (uint32_t)sw; a.sh = (uint32_t)sh; a.fw = (uint32_t)g.fw; a.fh = (uint32_t)g.fh;
    a.x0 = (uint32_t)g.x0; a.y0 = (uint32_t)g.y0; a.tw = (uint32_t)g.tw; a.th = (uint32_t)g.th;
    a.resize = (sw != g.tw || sh != g.th) ? 1u : 0u;
    a.wide = (dst_bytes >= (1ull << 31) || 2ull * a.tw * a.sw >= (1ull << 31) || 2ull * a.th * a.sh >= (1ull << 31)) ? 1u : 0u;       // as launch_compose
    a.div_row = to_dev(fastdiv(3u * a.fw)); a.div_fw = to_dev(fastdiv(a.fw)); a.div_tw2 = to_dev(fastdiv(2u * a.tw)); a.div_th2 = to_dev(fastdiv(2u * a.th));
    fa.src_stride = src_stride; fa.dst_stride = dst_stride;
    void* args[] = {(void*)&fa};
    HIPCHK(hipLaunchKernel((const void*)image_compose_frames_kernel, dim3((unsigned)((a.n_gran + 255u) / 256u), n_frames), dim3(256), args, 0, s));
    return T3_OK;
}
// what t3hip_encode_images_dev / t3hip_encode_images refuse before they ask for a device; fp, L: the batch encoder's plan of the composed frames
int check_encode_images(const void* src, int sw, int sh, uint64_t src_stride, uint32_t n_frames, int sub, int centered, const t3_cfg* cfg, const uint64_t* n_out,
                        Geo& g, t3_frames_plan& fp, t3_layout& L) {
    if (!cfg || !n_out) return T3_E_ARG;
    int rc = geometry(sub, centered, g); if (rc) return rc;
    if (sw >= 65536 || sh >= 65536) return T3_E_ARG;
    rc = plan_frames(0, (uint64_t)g.fw * g.fh, n_frames, *cfg, 2, fp, L); if (rc) return rc;
    const uint64_t src_bytes = sw > 0 && sh > 0 ? 3ull * (uint64_t)sw * (uint64_t)sh : 0;
    if (n_frames && src_bytes && !src) return T3_E_ARG;
    if (n_frames > 1 && src_stride < src_bytes) return T3_E_ARG;
    return T3_OK;
}
}  // namespace

extern "C" {

int t3hip_image_geometry(int sub, int centered, int* fw, int* fh, int* x0, int* y0, int* tw, int* th) {
    Geo g; const int rc = geometry(sub, centered, g); if (rc) return rc;
    if (fw) *fw = g.fw; if (fh) *fh = g.fh; if (x0) *x0 = g.x0; if (y0) *y0 = g.y0; if (tw) *tw = g.tw; if (th) *th = g.th;
    return T3_OK;
}

int t3hip_resize_rgb_nn_dev(const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    return launch_compose(d_src, sw, sh, d_dst, dw, dh, 0, 0, dw, dh, (hipStream_t)stream);
}
int t3hip_image_compose_dev(const uint8_t* d_src, int sw, int sh, int sub, int centered, uint8_t* d_frame_rgb, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    Geo g; const int rc = geometry(sub, centered, g); if (rc) return rc;
    return launch_compose(d_src, sw, sh, d_frame_rgb, g.fw, g.fh, g.x0, g.y0, g.tw, g.th, (hipStream_t)stream);
}
int t3hip_encode_image_dev(const uint8_t* d_src, int sw, int sh, int sub, int centered, const t3_cfg* cfg, void* d_out9, uint64_t cap_words,
                           uint64_t* n_out, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!cfg || !n_out) return T3_E_ARG;
    Geo g; int rc = geometry(sub, centered, g); if (rc) return rc;
    const uint64_t n_px = (uint64_t)g.fw * g.fh;
    void* d_frame; rc = scratch(c, Scratch::StreamImage, 3 * n_px + 64, &d_frame, (hipStream_t)stream); if (rc) return rc;
    rc = launch_compose(d_src, sw, sh, (uint8_t*)d_frame, g.fw, g.fh, g.x0, g.y0, g.tw, g.th, (hipStream_t)stream); if (rc) return rc;
    return t3hip_encode_rgb_dev((const uint8_t*)d_frame, n_px, cfg, d_out9, cap_words, n_out, stream);
}
int t3hip_decode_image_async(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, int sub, int centered, uint8_t* d_rgb, uint32_t* d_verdict, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    Geo g; const int rc = geometry(sub, centered, g); if (rc) return rc;
    return t3hip_decode_window_async(d_in9, n_in, cfg, (uint64_t)g.fw * g.fh / 2, (uint32_t)g.fw, (uint32_t)g.fh, (uint32_t)g.x0, (uint32_t)g.y0,
                                     (uint32_t)g.tw, (uint32_t)g.th, d_rgb, 2, d_verdict, stream);
}

// ---- batches of equal frames through the image front end: one compose launch, then the batch encoder; the batched window decode ----
int t3hip_encode_images_dev(const uint8_t* d_src, int sw, int sh, uint64_t src_stride, uint32_t n_frames, int sub, int centered, const t3_cfg* cfg, void* d_out9,
                            uint64_t out_stride, uint64_t* n_out, void* stream) {
    // what can be refused without a device is refused first (the batch rule, t3hip.h)
    Geo g; t3_frames_plan fp; t3_layout L;
    int rc = check_encode_images(d_src, sw, sh, src_stride, n_frames, sub, centered, cfg, n_out, g, fp, L); if (rc) return rc;
    *n_out = L.out_words;
    if (n_frames && L.out_words && !d_out9) return T3_E_ARG;
    if (n_frames > 1 && !frames_strides_ok(fp, nullptr, fp.in_stride_min, d_out9, out_stride)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (n_frames == 0) return T3_OK;
    const uint64_t stride = fp.in_stride_min;                                              // r16(fw * fh * 3)
    void* d_frames; rc = scratch(c, Scratch::StreamImage, (uint64_t)n_frames * stride + 64, &d_frames, (hipStream_t)stream); if (rc) return rc;
    rc = launch_compose_frames(d_src, sw, sh, src_stride, n_frames, (uint8_t*)d_frames, stride, g, (hipStream_t)stream); if (rc) return rc;
    return t3hip_encode_frames_dev(d_frames, (uint64_t)g.fw * g.fh, 2, stride, n_frames, cfg, d_out9, out_stride, n_out, stream);
}
int t3hip_decode_images_async(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, int sub, int centered, uint8_t* d_rgb,
                              uint64_t out_stride, uint32_t* d_verdict, void* stream) {
    Geo g; const int rc = geometry(sub, centered, g); if (rc) return rc;
    return t3hip_decode_frames_window_async(d_in9, n_in, in_stride, n_frames, cfg, (uint64_t)g.fw * g.fh / 2, (uint32_t)g.fw, (uint32_t)g.fh, (uint32_t)g.x0, (uint32_t)g.y0,
                                            (uint32_t)g.tw, (uint32_t)g.th, d_rgb, out_stride, 2, d_verdict, stream);
}

// ---- host-buffer forms (what include/ternary_codec_v6.hpp binds) ----
int t3hip_resize_rgb_nn(const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (dw < 0 || dh < 0) return T3_E_ARG;
    const uint64_t nb_in = sw > 0 && sh > 0 ? 3ull * (uint64_t)sw * (uint64_t)sh : 0, nb_out = 3ull * (uint64_t)dw * (uint64_t)dh;
    if (!nb_out) return T3_OK;
    if (!dst || (nb_in && !src)) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout; int rc = host_stage(c, src, nb_in, &di, nb_out, &dout); if (rc) return rc;
    rc = t3hip_resize_rgb_nn_dev((const uint8_t*)di, sw, sh, (uint8_t*)dout, dw, dh, c.stream); if (rc) return rc;
    return host_fetch(c, dst, dout, nb_out);
}
int t3hip_image_compose(const uint8_t* src, int sw, int sh, int sub, int centered, uint8_t* frame_rgb) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    Geo g; int rc = geometry(sub, centered, g); if (rc) return rc;
    const uint64_t nb_in = sw > 0 && sh > 0 ? 3ull * (uint64_t)sw * (uint64_t)sh : 0, nb_out = 3ull * (uint64_t)g.fw * (uint64_t)g.fh;
    if (!frame_rgb || (nb_in && !src)) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout; rc = host_stage(c, src, nb_in, &di, nb_out, &dout); if (rc) return rc;
    rc = t3hip_image_compose_dev((const uint8_t*)di, sw, sh, sub, centered, (uint8_t*)dout, c.stream); if (rc) return rc;
    return host_fetch(c, frame_rgb, dout, nb_out);
}

// host buffers with the device strides: one upload (the sources back to back at src_stride), the device entry, one download
int t3hip_encode_images(const uint8_t* src, int sw, int sh, uint64_t src_stride, uint32_t n_frames, int sub, int centered, const t3_cfg* cfg, void* out9,
                        uint64_t out_stride, uint64_t* n_out) {
    Geo g; t3_frames_plan fp; t3_layout L;
    int rc = check_encode_images(src, sw, sh, src_stride, n_frames, sub, centered, cfg, n_out, g, fp, L); if (rc) return rc;
    *n_out = L.out_words;
    if (n_frames && L.out_words && !out9) return T3_E_ARG;
    if (n_frames == 1) out_stride = fp.out_stride_min;
    else if (n_frames && !frames_strides_ok(fp, nullptr, fp.in_stride_min, nullptr, out_stride)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (n_frames == 0) return T3_OK;
    const uint64_t src_bytes = sw > 0 && sh > 0 ? 3ull * (uint64_t)sw * (uint64_t)sh : 0;
    if (n_frames == 1) src_stride = src_bytes;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout;
    rc = host_stage(c, src, src_bytes ? (uint64_t)(n_frames - 1) * src_stride + src_bytes : 0, &di, (uint64_t)n_frames * out_stride, &dout); if (rc) return rc;
    rc = t3hip_encode_images_dev((const uint8_t*)di, sw, sh, src_stride, n_frames, sub, centered, cfg, dout, out_stride, n_out, c.stream); if (rc) return rc;
    HIPCHK(copy_frames(out9, dout, out_stride, fp.out_bytes, n_frames, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return T3_OK;
}

}  // extern "C"
