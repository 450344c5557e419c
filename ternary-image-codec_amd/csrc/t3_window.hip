// t3_window.hip — window_crop_kernel (decoded run of pixels -> the w x h window, PixelYCbCrQuant or RGB8 out) and
// image_compose_kernel (RGB8 source -> nearest-neighbour resize + centring blit, the frame written once), and their forms over a batch
// of equal frames in one launch (window_crop_frames_kernel, image_compose_frames_kernel).  t3_window.h has the
// semantics; SURVEY §3.3, old/include/io_image.hpp:102-140 (resize_rgb_nn, blit_center_rgb), :184-235 (quant_stream_to_rgb,
// extract_center_q), :237-337 (the two flows).
//
// Both are pure byte streams (crop: 6 B in, 6 or 3 B out per window pixel; compose: 3 B out per frame pixel, up to 3 B in), so the
// shape is: one lane = one 16-byte store at a 16-byte aligned address, the source read as wide as its alignment allows.
//   crop     a window row starts on an even address (6-byte pixels): 16-byte loads at 2-byte alignment (as fast as aligned dwords,
//            DESIGN §5 fused decoder), 16 B per lane for pixels out, 36 B (six pixels, the 16 output bytes lie in their 18) for RGB
//   compose  a source row starts on any address: aligned dwords and v_alignbyte funnel shifts (16-byte loads at odd addresses are slow)
// A granule that crosses a row, touches the window's edge or the end of the stream, or is resized takes a per-pixel path; the first
// and the last granule of a destination that does not start / end on a 16-byte boundary store bytes.
// RGB out repeats t3_rgb.hip's quant_to_rgb_kernel step for step (same tables, same __fmul_rn / __fadd_rn order; -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_devutil.h"
#include "t3_window.h"

namespace t3 {

namespace {
struct __attribute__((packed, aligned(2))) V1a2w { uint32_t v; };
struct __attribute__((packed, aligned(2))) H1a2w { uint16_t v; };
__device__ __forceinline__ u32x4 load16e(const uint8_t* p) { return ((const U128a2*)p)->v; }      // p even
__device__ __forceinline__ uint32_t load4e(const uint8_t* p) { return ((const V1a2w*)p)->v; }
__device__ __forceinline__ uint32_t load2e(const uint8_t* p) { return ((const H1a2w*)p)->v; }

// n / d.d: multiply-shift (exact for n < 2^31, t3_host.cpp fastdiv) unless the launch is `wide`
__device__ __forceinline__ uint64_t qdiv(uint64_t n, const DevDiv& d, uint32_t wide) {
    if (d.d <= 1u) return n;
    return wide ? n / d.d : (uint64_t)(__umulhi((uint32_t)n, d.mul) >> d.sh);
}
__device__ __forceinline__ int lround_f(float x) {                 // std::lround: nearest, ties away from zero (t3_rgb.hip)
    const float t = truncf(x), f = __fsub_rn(x, t);
    return (int)t + (fabsf(f) >= 0.5f ? (x < 0.0f ? -1 : 1) : 0);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// one pixel record -> R | G << 8 | B << 16: dequantize_ycbcr io_image.hpp:79-84, ycbcr_to_rgb :57-66, as quant_to_rgb_kernel does them
__device__ __forceinline__ uint32_t px_to_rgb(uint32_t Yq, int Cbq, int Crq, const uint8_t* yd, const uint8_t* cd) {
    const int Y = Yq >= 242u ? 255 : yd[Yq];
    const int Cb = Cbq <= -40 ? 0 : (Cbq >= 40 ? 255 : cd[Cbq + 40]), Cr = Crq <= -40 ? 0 : (Crq >= 40 ? 255 : cd[Crq + 40]);
    const float y = (float)Y, cb = __fsub_rn((float)Cb, 128.0f), cr = __fsub_rn((float)Cr, 128.0f);
    const float r = __fadd_rn(y, __fmul_rn(1.402f, cr));
    const float g = __fsub_rn(__fsub_rn(y, __fmul_rn(0.344136f, cb)), __fmul_rn(0.714136f, cr));
    const float b = __fadd_rn(y, __fmul_rn(1.772f, cb));
    return (uint32_t)clampi(lround_f(r), 0, 255) | (uint32_t)clampi(lround_f(g), 0, 255) << 8 | (uint32_t)clampi(lround_f(b), 0, 255) << 16;
}
// six 24-bit pixels = 18 bytes; the 16 of them from byte r (0..2) on
__device__ __forceinline__ u32x4 bytes16_of(const uint32_t p[6], uint32_t r) {
    const uint32_t D0 = p[0] | p[1] << 24, D1 = p[1] >> 8 | p[2] << 16, D2 = p[2] >> 16 | p[3] << 8, D3 = p[4] | p[5] << 24, D4 = p[5] >> 8;
    u32x4 v;
    v.x = __builtin_amdgcn_alignbyte(D1, D0, r); v.y = __builtin_amdgcn_alignbyte(D2, D1, r);
    v.z = __builtin_amdgcn_alignbyte(D3, D2, r); v.w = __builtin_amdgcn_alignbyte(D4, D3, r);
    return v;
}
// a whole granule: one aligned 16-byte store
__device__ __forceinline__ void store16(uint8_t* out, uint64_t off, u32x4 v) { *(u32x4*)(out + off) = v; }
}  // namespace

// --------------------------------------------------------------------------------------------------------------------------
template <bool RGB>
__global__ __launch_bounds__(256) void window_crop_kernel(const WinCropArgs a) {
    __shared__ __attribute__((aligned(4))) uint8_t T[328];
    if constexpr (RGB) {
        for (uint32_t i = threadIdx.x; i < 82u; i += blockDim.x) ((uint32_t*)T)[i] = ((const uint32_t*)a.dq)[i];
        __syncthreads();
    }
    const uint8_t* const yd = T; const uint8_t* const cd = T + 244;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_gran) return;
    const int64_t q = (int64_t)(16u * g) - (int64_t)a.lead;                   // destination offset of the granule's first byte
    const bool whole = q >= 0 && (uint64_t)q + 16u <= a.out_bytes;
    // stream pixel of window pixel (x, y) and whether it exists; its bytes sit at run + 6 (s - first_px)
    auto src_of = [&](uint32_t y, uint32_t x, uint64_t& s) -> bool {
        const uint64_t row = (uint64_t)a.y0 + y;
        s = row * a.fw + a.x0 + x;
        return row < a.fh && s < a.stream_px;
    };
    if constexpr (!RGB) {
        if (whole) {
            const uint64_t H = (uint64_t)q >> 1;                              // halfword of the window (3 per pixel)
            const uint32_t rowh = 3u * a.w, y = (uint32_t)qdiv(H, a.div_row, a.wide), c = (uint32_t)(H - (uint64_t)y * rowh);
            if (c + 8u <= rowh) {
                uint64_t s0, s1; const bool v0 = src_of(y, c / 3u, s0), v1 = src_of(y, (c + 7u) / 3u, s1);
                if (v0 && v1) { store16(a.out, (uint64_t)q, load16e(a.run + 6u * (s0 - a.first_px) + 2u * (c % 3u))); return; }
                if (!v0) { const u32x4 z = {0u, 0u, 0u, 0u}; store16(a.out, (uint64_t)q, z); return; }   // (rows run forward: nothing behind an absent pixel)
            }
        }
        uint32_t hw[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const int64_t off = q + 2 * (int64_t)j; hw[j] = 0;
            if (off < 0 || (uint64_t)off >= a.out_bytes) continue;
            const uint64_t H = (uint64_t)off >> 1;
            const uint32_t rowh = 3u * a.w, y = (uint32_t)qdiv(H, a.div_row, a.wide), c = (uint32_t)(H - (uint64_t)y * rowh);
            uint64_t s;
            if (src_of(y, c / 3u, s)) hw[j] = load2e(a.run + 6u * (s - a.first_px) + 2u * (c % 3u));
        }
        if (whole) { const u32x4 v = {hw[0] | hw[1] << 16, hw[2] | hw[3] << 16, hw[4] | hw[5] << 16, hw[6] | hw[7] << 16}; store16(a.out, (uint64_t)q, v); return; }
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const int64_t off = q + 2 * (int64_t)j;
            if (off >= 0 && (uint64_t)off < a.out_bytes) *(uint16_t*)(a.out + off) = (uint16_t)hw[j];    // out is 4-byte aligned, off even
        }
    } else {
        auto rgb_of = [&](uint32_t y, uint32_t x) -> uint32_t {
            uint64_t s;
            if (!src_of(y, x, s)) return px_to_rgb(0u, 0, 0, yd, cd);           // a zero record through the bridge: (0, 0, 0)
            const uint8_t* p = a.run + 6u * (s - a.first_px);
            return px_to_rgb(load2e(p), (int16_t)load2e(p + 2), (int16_t)load2e(p + 4), yd, cd);
        };
        if (!whole) {
            for (uint32_t i = 0; i < 16u; ++i) {
                const int64_t off = q + (int64_t)i;
                if (off < 0 || (uint64_t)off >= a.out_bytes) continue;
                const uint64_t P = (uint64_t)off / 3u; const uint32_t comp = (uint32_t)((uint64_t)off - 3u * P);
                const uint32_t y = (uint32_t)qdiv(P, a.div_row, a.wide), x = (uint32_t)(P - (uint64_t)y * a.w);
                a.out[off] = (uint8_t)(rgb_of(y, x) >> (8u * comp));
            }
            return;
        }
        const uint64_t P0 = (uint64_t)q / 3u; const uint32_t r = (uint32_t)((uint64_t)q - 3u * P0);
        uint32_t y = (uint32_t)qdiv(P0, a.div_row, a.wide), x = (uint32_t)(P0 - (uint64_t)y * a.w);
        uint32_t p[6];
        uint64_t s0, s5;
        if (x + 6u <= a.w && src_of(y, x, s0) && src_of(y, x + 5u, s5)) {       // six pixels of one row, all there: 36 contiguous bytes
            const uint8_t* sp = a.run + 6u * (s0 - a.first_px);
            const u32x4 A = load16e(sp), B = load16e(sp + 16); const uint32_t Cw = load4e(sp + 32);
            const uint32_t d[9] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, Cw};
#pragma unroll
            for (int j = 0; j < 6; ++j) {                                        // pixel j = halfwords 3 j .. 3 j + 2
                const uint32_t h0 = 3 * j, h1 = h0 + 1, h2 = h0 + 2;
                const uint32_t Yq = (d[h0 >> 1] >> (16u * (h0 & 1u))) & 0xFFFFu;
                const int Cbq = (int16_t)(d[h1 >> 1] >> (16u * (h1 & 1u))), Crq = (int16_t)(d[h2 >> 1] >> (16u * (h2 & 1u)));
                p[j] = px_to_rgb(Yq, Cbq, Crq, yd, cd);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) { p[j] = rgb_of(y, x); if (++x == a.w) { x = 0; ++y; } }   // (pixel 5 is a window pixel: byte q + 15 - r lies in it)
        }
        store16(a.out, (uint64_t)q, bytes16_of(p, r));
    }
}
template __global__ void window_crop_kernel<false>(const WinCropArgs);
template __global__ void window_crop_kernel<true>(const WinCropArgs);

// --------------------------------------------------------------------------------------------------------------------------
// The two kernels over a batch of equal frames in one launch (t3_window.h): frame = blockIdx.y, lead = 0.  The granule logic is the
// single-frame kernels' text once more, not a function both share: those stay the code they were (image_compose_kernel, below, also
// stays the object's last kernel).
template <bool RGB>
__global__ __launch_bounds__(256) void window_crop_frames_kernel(const WinCropFramesArgs fa) {
    const WinCropArgs& a = fa.a;
    __shared__ __attribute__((aligned(4))) uint8_t T[328];
    if constexpr (RGB) {
        for (uint32_t i = threadIdx.x; i < 82u; i += blockDim.x) ((uint32_t*)T)[i] = ((const uint32_t*)a.dq)[i];
        __syncthreads();
    }
    const uint8_t* const yd = T; const uint8_t* const cd = T + 244;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_gran) return;
    const uint8_t* const run = a.run + (uint64_t)blockIdx.y * fa.run_stride; uint8_t* const out = a.out + (uint64_t)blockIdx.y * fa.out_stride;   // this frame's
    const int64_t q = (int64_t)(16u * g);                                     // destination offset of the granule's first byte (lead = 0)
    const bool whole = (uint64_t)q + 16u <= a.out_bytes;
    // stream pixel of window pixel (x, y) and whether it exists; its bytes sit at run + 6 (s - first_px)
    auto src_of = [&](uint32_t y, uint32_t x, uint64_t& s) -> bool {
        const uint64_t row = (uint64_t)a.y0 + y;
        s = row * a.fw + a.x0 + x;
        return row < a.fh && s < a.stream_px;
    };
    if constexpr (!RGB) {
        if (whole) {
            const uint64_t H = (uint64_t)q >> 1;                              // halfword of the window (3 per pixel)
            const uint32_t rowh = 3u * a.w, y = (uint32_t)qdiv(H, a.div_row, a.wide), c = (uint32_t)(H - (uint64_t)y * rowh);
            if (c + 8u <= rowh) {
                uint64_t s0, s1; const bool v0 = src_of(y, c / 3u, s0), v1 = src_of(y, (c + 7u) / 3u, s1);
                if (v0 && v1) { store16(out, (uint64_t)q, load16e(run + 6u * (s0 - a.first_px) + 2u * (c % 3u))); return; }
                if (!v0) { const u32x4 z = {0u, 0u, 0u, 0u}; store16(out, (uint64_t)q, z); return; }   // (rows run forward: nothing behind an absent pixel)
            }
        }
        uint32_t hw[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const int64_t off = q + 2 * (int64_t)j; hw[j] = 0;
            if (off < 0 || (uint64_t)off >= a.out_bytes) continue;
            const uint64_t H = (uint64_t)off >> 1;
            const uint32_t rowh = 3u * a.w, y = (uint32_t)qdiv(H, a.div_row, a.wide), c = (uint32_t)(H - (uint64_t)y * rowh);
            uint64_t s;
            if (src_of(y, c / 3u, s)) hw[j] = load2e(run + 6u * (s - a.first_px) + 2u * (c % 3u));
        }
        if (whole) { const u32x4 v = {hw[0] | hw[1] << 16, hw[2] | hw[3] << 16, hw[4] | hw[5] << 16, hw[6] | hw[7] << 16}; store16(out, (uint64_t)q, v); return; }
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const int64_t off = q + 2 * (int64_t)j;
            if (off >= 0 && (uint64_t)off < a.out_bytes) *(uint16_t*)(out + off) = (uint16_t)hw[j];    // out is 4-byte aligned, off even
        }
    } else {
        auto rgb_of = [&](uint32_t y, uint32_t x) -> uint32_t {
            uint64_t s;
            if (!src_of(y, x, s)) return px_to_rgb(0u, 0, 0, yd, cd);           // a zero record through the bridge: (0, 0, 0)
            const uint8_t* p = run + 6u * (s - a.first_px);
            return px_to_rgb(load2e(p), (int16_t)load2e(p + 2), (int16_t)load2e(p + 4), yd, cd);
        };
        if (!whole) {
            for (uint32_t i = 0; i < 16u; ++i) {
                const int64_t off = q + (int64_t)i;
                if (off < 0 || (uint64_t)off >= a.out_bytes) continue;
                const uint64_t P = (uint64_t)off / 3u; const uint32_t comp = (uint32_t)((uint64_t)off - 3u * P);
                const uint32_t y = (uint32_t)qdiv(P, a.div_row, a.wide), x = (uint32_t)(P - (uint64_t)y * a.w);
                out[off] = (uint8_t)(rgb_of(y, x) >> (8u * comp));
            }
            return;
        }
        const uint64_t P0 = (uint64_t)q / 3u; const uint32_t r = (uint32_t)((uint64_t)q - 3u * P0);
        uint32_t y = (uint32_t)qdiv(P0, a.div_row, a.wide), x = (uint32_t)(P0 - (uint64_t)y * a.w);
        uint32_t p[6];
        uint64_t s0, s5;
        if (x + 6u <= a.w && src_of(y, x, s0) && src_of(y, x + 5u, s5)) {       // six pixels of one row, all there: 36 contiguous bytes
            const uint8_t* sp = run + 6u * (s0 - a.first_px);
            const u32x4 A = load16e(sp), B = load16e(sp + 16); const uint32_t Cw = load4e(sp + 32);
            const uint32_t d[9] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, Cw};
#pragma unroll
            for (int j = 0; j < 6; ++j) {                                        // pixel j = halfwords 3 j .. 3 j + 2
                const uint32_t h0 = 3 * j, h1 = h0 + 1, h2 = h0 + 2;
                const uint32_t Yq = (d[h0 >> 1] >> (16u * (h0 & 1u))) & 0xFFFFu;
                const int Cbq = (int16_t)(d[h1 >> 1] >> (16u * (h1 & 1u))), Crq = (int16_t)(d[h2 >> 1] >> (16u * (h2 & 1u)));
                p[j] = px_to_rgb(Yq, Cbq, Crq, yd, cd);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) { p[j] = rgb_of(y, x); if (++x == a.w) { x = 0; ++y; } }   // (pixel 5 is a window pixel: byte q + 15 - r lies in it)
        }
        store16(out, (uint64_t)q, bytes16_of(p, r));
    }
}
template __global__ void window_crop_frames_kernel<false>(const WinCropFramesArgs);
template __global__ void window_crop_frames_kernel<true>(const WinCropFramesArgs);

__global__ __launch_bounds__(256) void image_compose_frames_kernel(const ComposeFramesArgs fa) {
    const ComposeArgs& a = fa.a;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_gran) return;
    const uint8_t* const src = a.src + (uint64_t)blockIdx.y * fa.src_stride; uint8_t* const dst = a.dst + (uint64_t)blockIdx.y * fa.dst_stride;   // this frame's
    const int64_t q = (int64_t)(16u * g);                                         // (lead = 0)
    // frame pixel (x, y) -> R | G << 8 | B << 16
    auto px_of = [&](uint32_t y, uint32_t x) -> uint32_t {
        const uint32_t ty = y - a.y0, tx = x - a.x0;                              // (wrap below the window: large, fails the test)
        if (ty >= a.th || tx >= a.tw) return 0u;
        uint32_t sy = ty, sx = tx;
        if (a.resize) {
            sy = (uint32_t)qdiv((uint64_t)(2u * ty + 1u) * a.sh, a.div_th2, a.wide);
            sx = (uint32_t)qdiv((uint64_t)(2u * tx + 1u) * a.sw, a.div_tw2, a.wide);
        }
        const uint8_t* p = src + 3u * ((uint64_t)sy * a.sw + sx);
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    };
    if (q < 0 || (uint64_t)q + 16u > a.dst_bytes) {
        for (uint32_t i = 0; i < 16u; ++i) {
            const int64_t off = q + (int64_t)i;
            if (off < 0 || (uint64_t)off >= a.dst_bytes) continue;
            const uint64_t P = (uint64_t)off / 3u; const uint32_t comp = (uint32_t)((uint64_t)off - 3u * P);
            const uint32_t y = (uint32_t)qdiv(P, a.div_fw, a.wide), x = (uint32_t)(P - (uint64_t)y * a.fw);
            dst[off] = (uint8_t)(px_of(y, x) >> (8u * comp));
        }
        return;
    }
    const uint64_t rowb = 3ull * a.fw;
    const uint32_t yb = (uint32_t)qdiv((uint64_t)q, a.div_row, a.wide); const uint64_t xb = (uint64_t)q - yb * rowb;
    if (xb + 16u <= rowb) {                                                        // one frame row
        const uint64_t wlo = 3ull * a.x0, whi = 3ull * ((uint64_t)a.x0 + a.tw);
        if (yb - a.y0 >= a.th || xb + 16u <= wlo || xb >= whi) { const u32x4 z = {0u, 0u, 0u, 0u}; store16(dst, (uint64_t)q, z); return; }
        if (!a.resize && xb >= wlo && xb + 16u <= whi) {                           // 16 source bytes in a row, at any address
            const uintptr_t A = (uintptr_t)(src + 3ull * (uint64_t)(yb - a.y0) * a.sw + (xb - wlo));
            const uint32_t* w = (const uint32_t*)(A & ~(uintptr_t)3); const uint32_t sh = (uint32_t)(A & 3u);
            const uint32_t W0 = w[0], W1 = w[1], W2 = w[2], W3 = w[3], W4 = sh ? w[4] : 0u;   // (the fifth dword only when bytes of it are wanted)
            const u32x4 v = {__builtin_amdgcn_alignbyte(W1, W0, sh), __builtin_amdgcn_alignbyte(W2, W1, sh), __builtin_amdgcn_alignbyte(W3, W2, sh), __builtin_amdgcn_alignbyte(W4, W3, sh)};
            store16(dst, (uint64_t)q, v); return;
        }
    }
    const uint64_t P0 = (uint64_t)q / 3u; const uint32_t r = (uint32_t)((uint64_t)q - 3u * P0);
    uint32_t y = (uint32_t)qdiv(P0, a.div_fw, a.wide), x = (uint32_t)(P0 - (uint64_t)y * a.fw);
    uint32_t p[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) { p[j] = px_of(y, x); if (++x == a.fw) { x = 0; ++y; } }   // (pixel 5 is a frame pixel: byte q + 15 - r lies in it)
    store16(dst, (uint64_t)q, bytes16_of(p, r));
}

// --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_compose_kernel(const ComposeArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_gran) return;
    const int64_t q = (int64_t)(16u * g) - (int64_t)a.lead;
    // frame pixel (x, y) -> R | G << 8 | B << 16
    auto px_of = [&](uint32_t y, uint32_t x) -> uint32_t {
        const uint32_t ty = y - a.y0, tx = x - a.x0;                              // (wrap below the window: large, fails the test)
        if (ty >= a.th || tx >= a.tw) return 0u;
        uint32_t sy = ty, sx = tx;
        if (a.resize) {
            sy = (uint32_t)qdiv((uint64_t)(2u * ty + 1u) * a.sh, a.div_th2, a.wide);
            sx = (uint32_t)qdiv((uint64_t)(2u * tx + 1u) * a.sw, a.div_tw2, a.wide);
        }
        const uint8_t* p = a.src + 3u * ((uint64_t)sy * a.sw + sx);
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    };
    if (q < 0 || (uint64_t)q + 16u > a.dst_bytes) {
        for (uint32_t i = 0; i < 16u; ++i) {
            const int64_t off = q + (int64_t)i;
            if (off < 0 || (uint64_t)off >= a.dst_bytes) continue;
            const uint64_t P = (uint64_t)off / 3u; const uint32_t comp = (uint32_t)((uint64_t)off - 3u * P);
            const uint32_t y = (uint32_t)qdiv(P, a.div_fw, a.wide), x = (uint32_t)(P - (uint64_t)y * a.fw);
            a.dst[off] = (uint8_t)(px_of(y, x) >> (8u * comp));
        }
        return;
    }
    const uint64_t rowb = 3ull * a.fw;
    const uint32_t yb = (uint32_t)qdiv((uint64_t)q, a.div_row, a.wide); const uint64_t xb = (uint64_t)q - yb * rowb;
    if (xb + 16u <= rowb) {                                                        // one frame row
        const uint64_t wlo = 3ull * a.x0, whi = 3ull * ((uint64_t)a.x0 + a.tw);
        if (yb - a.y0 >= a.th || xb + 16u <= wlo || xb >= whi) { const u32x4 z = {0u, 0u, 0u, 0u}; store16(a.dst, (uint64_t)q, z); return; }
        if (!a.resize && xb >= wlo && xb + 16u <= whi) {                           // 16 source bytes in a row, at any address
            const uintptr_t A = (uintptr_t)(a.src + 3ull * (uint64_t)(yb - a.y0) * a.sw + (xb - wlo));
            const uint32_t* w = (const uint32_t*)(A & ~(uintptr_t)3); const uint32_t sh = (uint32_t)(A & 3u);
            const uint32_t W0 = w[0], W1 = w[1], W2 = w[2], W3 = w[3], W4 = sh ? w[4] : 0u;   // (the fifth dword only when bytes of it are wanted)
            const u32x4 v = {__builtin_amdgcn_alignbyte(W1, W0, sh), __builtin_amdgcn_alignbyte(W2, W1, sh), __builtin_amdgcn_alignbyte(W3, W2, sh), __builtin_amdgcn_alignbyte(W4, W3, sh)};
            store16(a.dst, (uint64_t)q, v); return;
        }
    }
    const uint64_t P0 = (uint64_t)q / 3u; const uint32_t r = (uint32_t)((uint64_t)q - 3u * P0);
    uint32_t y = (uint32_t)qdiv(P0, a.div_fw, a.wide), x = (uint32_t)(P0 - (uint64_t)y * a.fw);
    uint32_t p[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) { p[j] = px_of(y, x); if (++x == a.fw) { x = 0; ++y; } }   // (pixel 5 is a frame pixel: byte q + 15 - r lies in it)
    store16(a.dst, (uint64_t)q, bytes16_of(p, r));
}

}  // namespace t3
