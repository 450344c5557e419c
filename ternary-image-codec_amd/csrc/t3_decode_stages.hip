// t3_decode_stages.hip — the reference decoder's stages 2 and 3 as kernels of their own, for callers that run them one at a time
// (descramble_words_inplace OLD:938-947, demap_and_rsdecode_bands_from_words OLD:948-993; t3_api_stages.cpp launches them).
// dec_gather_rs_kernel (t3_decode.hip) fuses both behind the header read and cannot decode a body that is already descrambled.
//
//   descramble_words_kernel  in place over 9 n bytes at any alignment: 16-byte accesses on the aligned interior, a byte per lane
//                            on the head and tail; byte i takes scrambler state pre0 / pre1 (i < 2), else cyc24's (i - 2) % 6 field
//                            (t3_host.cpp scrambler_cycle), so no lane waits for another
//   stage_decode_kernel      slot demap + RS decode of all nine bands of a descrambled body in one launch, per-band k and arithmetic.
//                            Workgroup g = nine waves, wave b = band b, lane l = block 64 g + l of that band.  Block m of every band
//                            but the beacon band is slot b of words [26 m, 26 m + 26), so the workgroup stages its 1664-word run in
//                            LDS with coalesced loads and every wave reads its band from there; the beacon band's blocks do not line
//                            up with word runs and its wave gathers them through the index map of dec_gather_rs_kernel's COMPAT
//                            branch.  rs_decode_block<R> (t3_rs_core.h) on LDS field tables; each wave stages its blocks' k data
//                            symbols, which are contiguous in the output, and stores them coalesced.  A failing block lowers *n_valid
//                            to its output offset (atomicMin): offsets grow in (band, block) order, so that minimum is the length of
//                            the prefix the reference leaves in out_syms when it returns false.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
#include "t3_decode.h"

namespace t3 {

// ---- descramble -------------------------------------------------------------------------------------------------------
// tab[256 st + s] = s with st subtracted from each of its three trits (descramble_symbol OLD:88-94; s reduced trit-wise as unpack3 does)
__device__ __forceinline__ void build_descr_table(uint8_t* tab) {
    for (uint32_t i = threadIdx.x; i < 768u; i += blockDim.x) {
        const uint32_t st = i >> 8, s = i & 255u;
        const uint32_t t0 = (s % 3u + 3u - st) % 3u, t1 = ((s / 3u) % 3u + 3u - st) % 3u, t2 = ((s / 9u) % 3u + 3u - st) % 3u;
        tab[i] = (uint8_t)(t0 + 3u * t1 + 9u * t2);
    }
}
__device__ __forceinline__ uint32_t mod6_u64(uint64_t x) {   // 2^32 = 4 (mod 6)
    return ((uint32_t)(x >> 32) % 6u * 4u + (uint32_t)x % 6u) % 6u;
}
// the states of bytes i0 .. i0 + 15, two bits each (byte q at bits 2q)
__device__ __forceinline__ uint32_t states16(uint64_t i0, const DescrArgs& a) {
    const uint64_t f = a.cyc24 & 0xFFFu, rep = f | f << 12 | f << 24 | f << 36;          // cyc[0..5] four times over: 48 bits
    if (i0 >= 2) return (uint32_t)(rep >> (2u * mod6_u64(i0 - 2)));
    const uint32_t pre = a.pre0 | a.pre1 << 2;
    return i0 == 0 ? pre | (uint32_t)(rep << 4) : a.pre1 | (uint32_t)(rep << 2);
}
__device__ __forceinline__ uint32_t state_of(uint64_t i, const DescrArgs& a) {
    if (i < 2) return i == 0 ? a.pre0 : a.pre1;
    return (a.cyc24 >> (2u * mod6_u64(i - 2))) & 3u;
}
__device__ __forceinline__ uint32_t descr_dword(const uint8_t* tab, uint32_t w, uint32_t st8) {   // four bytes, their states in st8
    uint32_t r = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) r |= (uint32_t)tab[((st8 >> (2 * q)) & 3u) << 8 | ((w >> (8 * q)) & 255u)] << (8 * q);
    return r;
}

__global__ __launch_bounds__(256) void descramble_words_kernel(const DescrArgs a) {
    __shared__ uint8_t tab[768];
    build_descr_table(tab);
    __syncthreads();
    uint8_t* p = a.words;
    const uint64_t n = a.n_bytes;
    const uint64_t head = min((uint64_t)((16u - ((uintptr_t)p & 15u)) & 15u), n);      // bytes in front of the first 16-byte boundary
    const uint64_t n16 = (n - head) / 16, tail0 = head + 16 * n16;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    v4* q16 = (v4*)(p + head);
    for (uint64_t c = tid; c < n16; c += 4 * stride) {                 // four 16-byte loads in flight per lane
        v4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const uint64_t j = c + u * stride; if (j < n16) v[u] = q16[j]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t j = c + u * stride;
            if (j >= n16) continue;
            const uint32_t st = states16(head + 16 * j, a);
            v4 o;
            o.x = descr_dword(tab, v[u].x, st); o.y = descr_dword(tab, v[u].y, st >> 8);
            o.z = descr_dword(tab, v[u].z, st >> 16); o.w = descr_dword(tab, v[u].w, st >> 24);
            q16[j] = o;
        }
    }
    if (tid < 32) {                                                     // head (< 16 bytes) and tail (< 16 bytes): a byte per lane
        const uint64_t i = tid < 16 ? tid : tail0 + (tid - 16);
        if ((tid < 16 && i < head) || (tid >= 16 && i < n)) p[i] = tab[state_of(i, a) << 8 | p[i]];
    }
}

// ---- slot demap + RS decode ---------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ bool stage_decode_one(const RsView& v, uint8_t* c, bool fixed) { return rs_decode_block<R>(v, c, fixed); }

__global__ __launch_bounds__(kStageThreads) void stage_decode_kernel(const StageDecArgs a) {
    __shared__ RsTables sT;
    __shared__ __attribute__((aligned(16))) uint8_t run[kStageRunBytes + 16];                  // the run, 16-byte phase of the body kept
    __shared__ __attribute__((aligned(16))) uint8_t ost[9][kStageBlocks * 24 + 16];            // per wave: its blocks' data symbols
    __shared__ uint8_t cw[kStageThreads * 26];                                                  // per lane: the block being corrected
    for (int i = threadIdx.x; i < (int)sizeof(RsTables); i += blockDim.x) ((uint8_t*)&sT)[i] = ((const uint8_t*)a.tab)[i];
    const uint64_t g = blockIdx.x;
    // stage words [1664 g, min(1664 (g + 1), 26 NB)) -- only the words of whole blocks of the non-beacon bands
    const uint64_t w_end = min((g + 1) * (uint64_t)(26 * kStageBlocks), 26 * a.nb);
    const uint64_t beg = 9 * g * (uint64_t)(26 * kStageBlocks), end = 9 * w_end;
    const uint32_t ph = (uint32_t)(((uintptr_t)a.body + beg) & 15u);     // every run starts at the same phase (14976 = 16 x 936)
    {
        const uint8_t* src = a.body + beg;
        const uint32_t len = (uint32_t)(end - beg), head = min((16u - ph) & 15u, len), n16 = (len - head) / 16, tail0 = head + 16 * n16;
        typedef uint32_t v4 __attribute__((ext_vector_type(4)));
        for (uint32_t c = threadIdx.x; c < n16; c += blockDim.x) *(v4*)(run + ph + head + 16 * c) = *(const v4*)(src + head + 16 * c);
        if (threadIdx.x < 16) { if (threadIdx.x < head) run[ph + threadIdx.x] = src[threadIdx.x]; }
        else if (threadIdx.x < 32 && tail0 + (threadIdx.x - 16) < len) run[ph + tail0 + threadIdx.x - 16] = src[tail0 + threadIdx.x - 16];
    }
    __syncthreads();
    const RsView v{sT.mul, sT.add, sT.neg, sT.inv, sT.exp};
    const uint32_t b = threadIdx.x >> 6, l = threadIdx.x & 63u;          // wave = band, lane = block of the run
    const bool bcn = b == a.bcn_band;
    const uint64_t nblk = bcn ? a.bcn_blocks : a.nb, m0 = g * kStageBlocks;
    if (m0 >= nblk) return;                                              // (no barrier follows: the waves part here)
    const uint32_t cnt = (uint32_t)min((uint64_t)kStageBlocks, nblk - m0);
    const uint32_t k = a.band_k[b];
    uint8_t* dst = a.out + a.band_off[b] + m0 * k;
    const uint32_t oph = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t* os = ost[b] + oph;                                          // the wave's staging, same 16-byte phase as dst
    if (l < cnt) {
        uint8_t* c = cw + 26u * threadIdx.x;                            // (in registers it would be indexed at run time: scratch)
        if (!bcn) {
            const uint8_t* s = run + ph + 234u * l + b;
#pragma unroll
            for (int i = 0; i < 26; ++i) c[i] = s[9 * i] % 27u;
        } else {
            // beacon band: symbol j is slot b of word j + j / (period - 1) + 1 (period >= 2 here, else the band is empty)
#pragma unroll
            for (int i = 0; i < 26; ++i) {
                const uint64_t j = 26 * (m0 + l) + i;
                const uint64_t q = j < (1ull << 31) ? (uint64_t)((__umulhi((uint32_t)j, a.div_p1.mul) >> a.div_p1.sh)) : j / a.div_p1.d;
                c[i] = a.body[9 * (j + (a.div_p1.d <= 1 ? j : q) + 1) + b] % 27u;
            }
        }
        const bool fixed = a.band_fixed[b] != 0;
        bool ok;
        switch (k) {
            case 24: ok = stage_decode_one<2>(v, c, fixed); break;
            case 22: ok = stage_decode_one<4>(v, c, fixed); break;
            case 20: ok = stage_decode_one<6>(v, c, fixed); break;
            default: ok = stage_decode_one<8>(v, c, fixed); break;
        }
        if (!ok) atomicMin((unsigned long long*)a.n_valid, (unsigned long long)(a.band_off[b] + (m0 + l) * k));
#pragma unroll
        for (uint32_t p = 0; p < 24; ++p) if (p < k) os[l * k + p] = c[p];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");           // the wave's staged symbols, visible to its own lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // the wave's cnt * k bytes: 16-byte stores on dst's aligned interior, a byte per lane on its head and tail
    const uint32_t len = cnt * k, head = min((16u - oph) & 15u, len), n16 = (len - head) / 16, tail0 = head + 16 * n16;
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    for (uint32_t c = l; c < n16; c += 64) *(v4*)(dst + head + 16 * c) = *(const v4*)(os + head + 16 * c);
    if (l < 16) { if (l < head) dst[l] = os[l]; }
    else if (l < 32 && tail0 + (l - 16) < len) dst[tail0 + l - 16] = os[tail0 + l - 16];
}

__global__ void fill_u64_kernel(uint64_t* p, uint64_t v) { *p = v; }

}  // namespace t3
