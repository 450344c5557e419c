// t3_window.h — the window decode's crop and the image front end's compose, for one frame and for a batch of equal frames (t3_window.hip;
// host side: t3_api_decode.cpp, t3_api_image.cpp).  The kernels are byte streams: one lane = one 16-byte granule of the destination at a 16-byte aligned ADDRESS
// (the destination pointer itself is only 4-byte aligned: granule g covers destination offsets [16 g - lead, 16 g - lead + 16)).
#pragma once
#include <stdint.h>

#include "t3_device.h"

namespace t3 {

// window_crop_kernel: `run` holds the decoded pixels [first_px, first_px + ...) of a frame read as rows of fw pixels (6 bytes each, run
// 2-byte aligned at least); output pixel (x, y) of the w x h window is stream pixel (y0 + y) fw + x0 + x, or a zero record when its row
// is >= fh or the pixel is >= stream_px.  The host guarantees that every other pixel the window names lies in the run.
struct WinCropArgs {
    const uint8_t* run; uint8_t* out;
    const uint8_t* dq;              // RGB out: dequantiser tables yd[244] | cd[84] (t3_rgb.h), else unused
    uint64_t first_px, stream_px;
    uint64_t out_bytes;             // 6 w h or 3 w h
    uint64_t n_gran;                // 16-byte granules the destination touches
    uint32_t fw, fh, x0, y0, w, h;
    uint32_t lead;                  // (address of out) mod 16
    uint32_t wide;                  // out_bytes >= 2^31: 64-bit divisions instead of the multiply-shift ones
    DevDiv div_row;                 // by the window row's units: 3 w halfwords (pixels out) / w pixels (RGB out)
};
// image_compose_kernel: a fw x fh RGB8 frame written once; frame pixel (x, y) inside the target window [x0, x0 + tw) x [y0, y0 + th) is
// source pixel (sy, sx) = (floor((2 (y - y0) + 1) sh / (2 th)), floor((2 (x - x0) + 1) sw / (2 tw))) -- resize_rgb_nn,
// io_image.hpp:102-124, in integers; the identity when the source has the target's size -- every other frame pixel is zero.
struct ComposeArgs {
    const uint8_t* src; uint8_t* dst;
    uint64_t dst_bytes, n_gran;
    uint32_t sw, sh, fw, fh, x0, y0, tw, th;
    uint32_t lead, wide;            // wide: dst_bytes >= 2^31 or a resize product >= 2^31
    uint32_t resize;                // 0: sw == tw and sh == th
    DevDiv div_row;                 // by 3 fw (frame row bytes)
    DevDiv div_fw;                  // by fw
    DevDiv div_tw2, div_th2;        // by 2 tw, 2 th
};
// The two kernels over a batch of equal frames in one launch (frame = blockIdx.y, so 65535 frames at most): `a` is one frame's argument
// block with lead = 0 -- every frame's destination starts on a 16-byte boundary -- and frame f reads a.run / a.src + f * the source
// stride and writes a.out / a.dst + f * the destination stride (a multiple of 16).  Bytes of a stride behind a frame's own are not written.
struct WinCropFramesArgs { WinCropArgs a; uint64_t run_stride, out_stride; };
struct ComposeFramesArgs { ComposeArgs a; uint64_t src_stride, dst_stride; };
#if defined(__HIPCC__)
template <bool RGB> __global__ void window_crop_kernel(const WinCropArgs a);
__global__ void image_compose_kernel(const ComposeArgs a);
template <bool RGB> __global__ void window_crop_frames_kernel(const WinCropFramesArgs fa);
__global__ void image_compose_frames_kernel(const ComposeFramesArgs fa);
#endif
}  // namespace t3
