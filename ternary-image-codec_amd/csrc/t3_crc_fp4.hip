// t3_crc_fp4.hip — CRC-32 of the coded payload on the matrix cores (crc32_acc, src/io_t3p_t3v.cpp:20-36; the T3V frame index and the
// payload CRC of the containers), on the block-scaled FP4 instruction of gfx950.
//
// The CRC register update is GF(2)-linear, so the remainder of a 64-byte chunk is a 32 x 512 bit matrix (A, host-built in slices) times
// the chunk's bits.  Column n of the B operand = chunk n of the wave's current 2 KiB: a wave reads 2 KiB per round perfectly coalesced
// (lane (n, h) takes bytes 64 n + 32 h .. + 32).  The column's running remainder re-enters as more K inputs through the feedback slice,
// an "append zero bytes" matrix over the distance to the column's next chunk.  After the last round a column's remainder moves to the end
// of the stream: 64 (31 - n) bytes per column (five masked steps through the "append 64 * 2^b bytes" slices), then, XOR-reduced over
// the columns, the common distance with one operator column per lane.  v_mfma_scale_f32_32x32x64_f8f6f4
// with FP4 (e2m1) operands runs 64 K values per instruction in the cycles the i8 instruction needs for 32: a 2 KiB round is 8 data
// instructions + 1 feedback instead of 16 + 1.  Block scales 2^0 (e8m0 127); every product is 0 or exactly 1, a dot product is at most
// 512 + 16, exact in f32; the remainder bit is the parity of its integer value.
// Round 3: no table, no LDS in the loop.  An input dword becomes its four B dwords with five vector instructions: w & 0x11111111,
// w & 0x22222222, w & 0x44444444 and (w >> 1) & 0x44444444 -- a bit stays where it is inside its nibble and therefore reads as FP4 0.5, 1.0
// or 2.0; the matrix slice holds the reciprocal weight (2.0, 1.0, 0.5) in that K slot, so the product is 1.  (Round 2 read a 256-entry
// byte -> eight-nibble table, 32 bank copies: two vector instructions + one LDS read per BYTE, and the compiler's schedule put the LDS
// latency of every step in series with its matrix instruction: ~1,100 cycles per round and SIMD.)  Which K slot carries which bit is free
// (the hardware pairs position p of lane half kh in A with the same position in B): the host builds the slices in the order the
// kernel feeds bits (t3_api_record.cpp, crc_init).
// Parity without a conversion: x = acc + 2^(23 - s) has the integer's bit 0 at mantissa bit s (the sum is exact: acc < 2^11); with
// s = 0, 4, 8, 12 for the four accumulators of a group the bits land in nibbles 0..3 of one dword at nibble bit 0 (FP4 0.5, weight 2.0 in
// the feedback slice): a packed add per two accumulators and one v_and_or per accumulator.
// The kernel's text is t3_crc_fp4_body.inc (device helpers: t3_crc_fp4_body.h): crc_fp4_frames_kernel (t3_crc_frames.hip) runs the same
// rounds on one of N equal streams.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
#include "t3_crc.h"
#include "t3_crc_fp4_body.h"

namespace t3 {

__global__ __launch_bounds__(256) void crc_fp4_kernel(const CrcMArgs a) {
#define T3_CRC_STREAM(p) (p)
#define T3_CRC_SLOT(p) (p)
#include "t3_crc_fp4_body.inc"
#undef T3_CRC_STREAM
#undef T3_CRC_SLOT
}

}  // namespace t3
