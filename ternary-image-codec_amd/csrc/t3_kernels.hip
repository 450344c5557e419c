// t3_kernels.hip — the small gfx950 (CDNA4, wave64) kernels of the Word27 encode path; the fused encoder K2 is t3_encode.h, compiled
// per front end by t3_encode_px.hip, t3_encode_words.hip and t3_encode_rgb.hip.
//
//   K1 pack_pixels_kernel     pixels -> raw Word27                       (encode_raw_pixels_to_words OLD:723-734)
//   K5 unpack_words_kernel    raw Word27 -> pixels                       (decode_raw_words_to_pixels OLD:735-747)
//      beacon_kernel          sparse beacon insertion pass               (OLD:1118-1141)
//      interleave_kernel      standalone 2-D boustrophedon               (OLD:750-813)
//      rs_encode_blocks_kernel  block-level RSCodec::encode_block        (OLD:517-535)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_device.h"
#include "t3_devutil.h"
#include "t3_enc_convert.h"
#include "t3_rs_core.h"

namespace t3 {

// ---------------------------------------------------------------------------------------------------------
// K1 / K5 : RAW packer (2 pixels <-> 9 symbols), one lane per word
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void px2_to_word(const uint32_t* c /*6 reduced comps*/, uint32_t* s /*9*/) {
    // T[0..4]=Ya T[5..8]=Cba T[9..12]=Cra T[13..17]=Yb T[18..21]=Cbb T[22..25]=Crb T[26]=0 (OLD:693-705)
    const uint32_t Y0 = c[0], B0 = c[1], R0 = c[2], Y1 = c[3], B1 = c[4], R1 = c[5];
    s[0] = mod27(Y0); s[1] = div27(Y0) + 9u * mod3(B0); s[2] = div3(B0); s[3] = mod27(R0);
    s[4] = div27(R0) + 3u * mod9(Y1); s[5] = div9(Y1); s[6] = mod27(B1); s[7] = div27(B1) + 3u * mod9(R1);
    s[8] = div9(R1);
}

// One lane = four words: 48 bytes of pixels in (three 16-byte loads), 36 bytes out (nine dwords); the frame's last lanes and
// unaligned buffers go element by element.
__device__ __forceinline__ void pack_one(const uint16_t* h /*6 components; nullptr-free*/, uint32_t n_valid_px, uint32_t* s) {
    uint32_t c[6];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if ((uint32_t)i < n_valid_px) { c[3 * i] = red_y(h[3 * i]); c[3 * i + 1] = red_c(h[3 * i + 1]); c[3 * i + 2] = red_c(h[3 * i + 2]); }
        else { c[3 * i] = 0; c[3 * i + 1] = 40; c[3 * i + 2] = 40; }     // PixelYCbCrQuant{} pad (OLD:730)
    }
    px2_to_word(c, s);
}
__global__ __launch_bounds__(256) void pack_pixels_kernel(const uint16_t* __restrict__ px, uint64_t n_px, uint8_t* __restrict__ words, uint64_t n_words) {
    const uint64_t w0 = 4 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (w0 >= n_words) return;
    if (2 * w0 + 8 <= n_px && w0 + 4 <= n_words && (((uintptr_t)px | (uintptr_t)words) & 15u) == 0) {
        uint32_t in[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) { const uint4 v = *(const uint4*)(px + 6 * w0 + 8 * k); in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w; }
        uint32_t o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            uint16_t h[6];
#pragma unroll
            for (uint32_t i = 0; i < 6; ++i) { const uint32_t e = 6u * q + i; h[i] = (uint16_t)(in[e >> 1] >> (16u * (e & 1u))); }
            uint32_t sy[9]; pack_one(h, 2, sy);
#pragma unroll
            for (uint32_t i = 0; i < 9; ++i) { const uint32_t b = 9u * q + i; o[b >> 2] |= (sy[i] & 0xFFu) << (8u * (b & 3u)); }
        }
        uint32_t* d = (uint32_t*)(words + 9 * w0);
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k] = o[k];
        return;
    }
    for (uint64_t w = w0; w < min(w0 + 4, n_words); ++w) {
        uint16_t h[6] = {0, 0, 0, 0, 0, 0};
        const uint32_t nv = (uint32_t)min((uint64_t)2, n_px > 2 * w ? n_px - 2 * w : 0ull);
        for (uint32_t i = 0; i < 3u * nv; ++i) h[i] = px[6 * w + i];
        uint32_t sy[9]; pack_one(h, nv, sy);
        for (int i = 0; i < 9; ++i) words[9 * w + i] = (uint8_t)sy[i];
    }
}

__device__ __forceinline__ void unpack_one(const uint32_t* craw, uint16_t* o) {
    uint32_t c[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = mod27(craw[i]);                     // unpack3 reduces each digit (OLD:28-31)
    // inverse of px2_to_word; trit 26 (= c[8]/9) is ignored (OLD:716-721)
    const uint32_t Y0 = c[0] + 27u * mod9(c[1]);
    const uint32_t B0 = div9(c[1]) + 3u * c[2];
    const uint32_t R0 = c[3] + 27u * mod3(c[4]);
    const uint32_t Y1 = div3(c[4]) + 9u * c[5];
    const uint32_t B1 = c[6] + 27u * mod3(c[7]);
    const uint32_t R1 = div3(c[7]) + 9u * mod9(c[8]);
    o[0] = (uint16_t)Y0; o[1] = (uint16_t)(int16_t)((int)B0 - 40); o[2] = (uint16_t)(int16_t)((int)R0 - 40);
    o[3] = (uint16_t)Y1; o[4] = (uint16_t)(int16_t)((int)B1 - 40); o[5] = (uint16_t)(int16_t)((int)R1 - 40);
}
// One lane = four words: nine dwords in, three 16-byte stores of pixels out.
__global__ __launch_bounds__(256) void unpack_words_kernel(const uint8_t* __restrict__ words, uint64_t n_words, uint16_t* __restrict__ px) {
    const uint64_t w0 = 4 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (w0 >= n_words) return;
    if (w0 + 4 <= n_words && (((uintptr_t)px | (uintptr_t)words) & 15u) == 0) {
        uint32_t in[9];
        const uint32_t* sdw = (const uint32_t*)(words + 9 * w0);
#pragma unroll
        for (int k = 0; k < 9; ++k) in[k] = sdw[k];
        uint32_t o[12];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            uint32_t c[9];
#pragma unroll
            for (uint32_t i = 0; i < 9; ++i) { const uint32_t b = 9u * q + i; c[i] = (in[b >> 2] >> (8u * (b & 3u))) & 0xFFu; }
            uint16_t h[6]; unpack_one(c, h);
#pragma unroll
            for (uint32_t i = 0; i < 3; ++i) o[3u * q + i] = (uint32_t)h[2 * i] | (uint32_t)h[2 * i + 1] << 16;
        }
        uint4* d = (uint4*)(px + 6 * w0);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        return;
    }
    for (uint64_t w = w0; w < min(w0 + 4, n_words); ++w) {
        uint32_t c[9];
        for (int i = 0; i < 9; ++i) c[i] = words[9 * w + i];
        uint16_t h[6]; unpack_one(c, h);
        for (int i = 0; i < 6; ++i) px[6 * w + i] = h[i];
    }
}

// ---------------------------------------------------------------------------------------------------------
// beacon insertion pass (OLD:1118-1141): framed[q] = beacon symbol at slot `slot` of every period-th word, else
// body[q - #beacons before q], zero past the body.  One lane = one 16-byte granule of the output frame: between two
// beacons that is a shifted copy (aligned dword loads + funnel shifts, one 16-byte store); a granule that holds a beacon
// or touches the header / the end of the body goes byte by byte.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beacon_kernel(const BeaconArgs a) {
    const uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g0 == 0) {
        for (uint32_t i = 0; i < a.hdr_syms; ++i) a.frame_out[i] = a.hdr[i];
        for (uint32_t i = 0; i < a.pad_bytes; ++i) a.frame_out[a.hdr_syms + a.framed_syms + i] = 0;
    }
    const uint64_t cyc = 9ull * a.period;
    const uint64_t end = a.hdr_syms + a.framed_syms;
    const bool small = end < (1ull << 32) && cyc < (1ull << 32);                  // 32-bit divisions where the frame allows
    auto before = [&](uint64_t q) -> uint64_t {                                    // beacons strictly before q
        if (a.slot >= 9u || q <= a.slot) return 0u;
        return small ? (uint64_t)(((uint32_t)q - a.slot - 1u) / (uint32_t)cyc + 1u) : (q - a.slot - 1u) / cyc + 1u;
    };
    for (uint64_t g = g0; 16 * g < end; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t B0 = 16 * g;
        if (B0 >= a.hdr_syms && B0 + 16 <= end && ((uintptr_t)a.frame_out & 15u) == 0) {
            const uint64_t q = B0 - a.hdr_syms, nb = before(q);
            if (nb == before(q + 16) && q - nb + 20 <= a.body_syms) {
                const uint8_t* src = a.body + (q - nb);
                const uint32_t sh = ((uint32_t)(uintptr_t)src & 3u) * 8u;
                const uint32_t* p = (const uint32_t*)((uintptr_t)src & ~(uintptr_t)3);
                uint32_t dw[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) dw[i] = p[i];
                *(uint4*)(a.frame_out + B0) = make_uint4(__builtin_amdgcn_alignbit(dw[1], dw[0], sh), __builtin_amdgcn_alignbit(dw[2], dw[1], sh),
                                                          __builtin_amdgcn_alignbit(dw[3], dw[2], sh), __builtin_amdgcn_alignbit(dw[4], dw[3], sh));
                continue;
            }
        }
        // byte by byte, no division per byte: the beacons are at slot + j cyc, `nb` of them lie before q
        const uint64_t Bs = max(B0, (uint64_t)a.hdr_syms), Be = min(B0 + 16, end);
        uint64_t nb = before(Bs - a.hdr_syms), qb = a.slot < 9u ? a.slot + nb * cyc : ~0ull;
        for (uint64_t B = Bs; B < Be; ++B) {
            const uint64_t q = B - a.hdr_syms;
            uint8_t v;
            if (q == qb) { v = (uint8_t)a.sym; ++nb; qb += cyc; }
            else { const uint64_t kq = q - nb; v = kq < a.body_syms ? a.body[kq] : 0; }
            a.frame_out[B] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// standalone 2-D boustrophedon (interleave2D_boustrophedon / deinterleave2D_boustrophedon OLD:750-813): out[u] = in[perm(u)].
// The map is an involution inside every row segment (odd rows of a chunk reversed, the stream's ragged last rows within
// their own length), so one kernel serves both directions.  API completeness: the frame kernels carry the map fused.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void interleave_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n, uint32_t w, uint32_t A, DevDiv div_A, DevDiv div_w) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const uint32_t chunk = div_any(u, div_A), base = chunk * A, rem = u - base, take = min(A, n - base);
    const uint32_t r = div_any(rem, div_w), c = rem - r * w, rowlen = min(w, take - r * w);
    out[u] = in[base + r * w + ((r & 1u) ? rowlen - 1u - c : c)];
}

// ---------------------------------------------------------------------------------------------------------
// block-level RS encode (RSCodec::encode_block OLD:517-535): out = data || data * P
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rs_encode_blocks_kernel(const uint8_t* __restrict__ data, uint64_t n_blocks, int k,
                                                               const uint8_t* __restrict__ P /*k x r*/, const RsTables* __restrict__ tab,
                                                               uint8_t* __restrict__ code) {
    __shared__ uint8_t sP[24 * 8]; __shared__ RsTables sT;
    const int r = 26 - k;
    for (int i = threadIdx.x; i < k * r; i += blockDim.x) sP[i] = P[i];
    for (int i = threadIdx.x; i < (int)sizeof(RsTables); i += blockDim.x) ((uint8_t*)&sT)[i] = ((const uint8_t*)tab)[i];
    __syncthreads();
    const uint64_t blk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= n_blocks) return;
    uint8_t par[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t* d = data + blk * k; uint8_t* o = code + blk * 26;
    for (int i = 0; i < k; ++i) {
        const uint8_t di = d[i] % 27u; o[i] = d[i];
        for (int j = 0; j < r; ++j) par[j] = sT.add[par[j] * 27 + sT.mul[di * 27 + sP[i * r + j]]];
    }
    for (int j = 0; j < r; ++j) o[k + j] = par[j];
}

}  // namespace t3
