// t3_devutil.h — device-only helpers with one definition each, shared by the encoder (t3_encode.h, t3_kernels.hip) and the decoders
// (t3_decode_fx.h, t3_decode_fx2.h, t3_decode_wg.h, t3_decode*.hip): the LDS array and its access by absolute address, small
// divisions by multiply-shift, division by a host-prepared DevDiv, the LDS barrier, 2-byte-aligned vector accesses, the
// interleave's row geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_device.h"

namespace t3 {

extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
// LDS access by absolute byte address.  The kernels own the whole LDS allocation (no static __shared__), so the dynamic
// array starts at address 0; going through `lds + x` instead makes the compiler add that (link-time) zero to every address.
#define T3_LDS(T, a) ((__attribute__((address_space(3))) T*)(uintptr_t)(a))
__device__ __forceinline__ uint32_t lds_u8(uint32_t a)  { return *T3_LDS(const uint8_t, a); }
__device__ __forceinline__ uint32_t lds_u32(uint32_t a) { return *T3_LDS(const uint32_t, a); }
// workgroup barrier behind this wave's LDS traffic only: loads and stores to memory stay in flight across it
__device__ __forceinline__ void barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
// 8 / 16 bytes at an address that is only AL-byte aligned, as one access (2-byte aligned: measured as fast as 16-byte aligned; odd
// addresses are not)
template <int AL> struct __attribute__((packed, aligned(AL))) U64a { u32x2 v; };
template <int AL> struct __attribute__((packed, aligned(AL))) U128a { u32x4 v; };
typedef U64a<2> U64a2;
typedef U128a<2> U128a2;
// The coded stream is read once: non-temporal loads (measured: clean stream 0.140 -> 0.131 ms, with errors 0.157 -> 0.154; non-temporal
// *stores* of the pixels cost 40 %: 0.140 -> 0.193).  p: 2-byte aligned
__device__ __forceinline__ u32x4 load16(const uint8_t* p) { return __builtin_nontemporal_load(&((const U128a2*)p)->v); }
// a 16-byte granule with its bytes in reverse order (uint4 or u32x4)
template <class V> __device__ __forceinline__ V rev16(const V q) {
    V r; r.x = __builtin_bswap32(q.w); r.y = __builtin_bswap32(q.z); r.z = __builtin_bswap32(q.y); r.w = __builtin_bswap32(q.x);
    return r;
}

// ---------------------------------------------------------------------------------------------------------
// small-integer division by powers of three with full-rate 24-bit multiplies (ranges checked in tests/test_host_logic.py)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t div3(uint32_t x)  { return __umul24(x, 171u) >> 9; }    // x < 512
__device__ __forceinline__ uint32_t div9(uint32_t x)  { return __umul24(x, 228u) >> 11; }   // x < 512
__device__ __forceinline__ uint32_t div27(uint32_t x) { return __umul24(x, 152u) >> 12; }   // x < 512
__device__ __forceinline__ uint32_t div81(uint32_t x) { return __umul24(x, 405u) >> 15; }   // x < 885
__device__ __forceinline__ uint32_t mod3(uint32_t x)  { return x - 3u * div3(x); }
__device__ __forceinline__ uint32_t mod9(uint32_t x)  { return x - 9u * div9(x); }
__device__ __forceinline__ uint32_t mod27(uint32_t x) { return x - 27u * div27(x); }
// two 16-bit values at once (packed 16-bit multiply and shift)
__device__ __forceinline__ u16x2 pk_d3(u16x2 x)  { return (x * (uint16_t)171) >> (uint16_t)9; }    // x < 512 (products < 2^16 for x <= 383)
__device__ __forceinline__ u16x2 pk_d9(u16x2 x)  { return (x * (uint16_t)228) >> (uint16_t)11; }   // x <= 287
__device__ __forceinline__ u16x2 pk_d27(u16x2 x) { return (x * (uint16_t)152) >> (uint16_t)12; }   // x <= 431
__device__ __forceinline__ uint32_t pk_bits(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
// x mod 3 for any 32-bit x
__device__ __forceinline__ uint32_t mod3_u32(uint32_t x) { return x - 3u * (uint32_t)(((uint64_t)x * 0xAAAAAAABull) >> 33); }
// SWAR reduction mod 3 of five 6-bit fields (each <= 63) to {0,1,2}: 4 == 1 (mod 3) so fold the high bits down.
__device__ __forceinline__ uint32_t mod3x5(uint32_t x) {
    x = (x & 0x030C30C3u) + ((x >> 2) & 0x0F3CF3CFu);   // <= 3 + 15
    x = (x & 0x030C30C3u) + ((x >> 2) & 0x030C30C3u);   // <= 3 + 3   (x <= 15 -> x>>2 <= 3)
    x = (x & 0x030C30C3u) + ((x >> 2) & 0x01041041u);   // <= 3
    const uint32_t t = x & (x >> 1) & 0x01041041u;      // fields equal to 3
    return x - (t | (t << 1));
}

// n / d for a DevDiv of the host (t3_host.hpp).  div_any: every d -- the multiply-shift is wrong for d <= 1, which is tested for.
// div_ge2: divisors known to be >= 2 (2-D geometry: the host takes rows of one symbol, where the map is the identity, as 1-D).  No test on
// d: hoisted out of the encoder's tile loop that test lived in a register pair the kernels did not have, was parked in a VGPR, spilled, and
// its reload (scratch_load + s_waitcnt vmcnt(0)) drained the next tile's prefetch in the middle of phase 1.
__device__ __forceinline__ uint32_t div_any(uint32_t n, const DevDiv& d) { return d.d <= 1 ? n : (__umulhi(n, d.mul) >> d.sh); }
__device__ __forceinline__ uint32_t div_ge2(uint32_t n, const DevDiv& d) { return __umulhi(n, d.mul) >> d.sh; }

// Row of the 2-D boustrophedon interleave that holds position v < n_sym (OLD:750-813: chunks of il_A = w h symbols, rows of il_w, the
// stream's ragged last chunk / row within their own length): start, length, parity (odd rows are reversed; the map is an involution
// inside a row, so pre- and post-interleave positions have the same row).  DIV: div_any or div_ge2.
struct IlRow { uint32_t start, len, odd; };
template <uint32_t (*DIV)(uint32_t, const DevDiv&)>
__device__ __forceinline__ IlRow il_row_of(const uint32_t v, const uint32_t n_sym, const uint32_t il_w, const uint32_t il_A, const DevDiv& div_A, const DevDiv& div_w) {
    const uint32_t chunk = DIV(v, div_A), base = chunk * il_A, rem = v - base, take = min(il_A, n_sym - base);
    const uint32_t r = DIV(rem, div_w), rw = r * il_w;
    IlRow g; g.start = base + rw; g.len = min(il_w, take - rw); g.odd = r & 1u;
    return g;
}

}  // namespace t3
