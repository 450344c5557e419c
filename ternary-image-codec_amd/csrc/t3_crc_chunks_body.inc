// t3_crc_chunks_body.inc -- the body of the table CRC-32 kernels, included by crc_chunks_kernel (t3_decode.hip: one stream) and
// crc_chunks_frames_kernel (t3_crc_frames.hip: blockIdx.y = one of N equal streams).  `a` is the stream's CrcArgs; text inside the kernels
// and the two macros T3_CRC_STREAM / T3_CRC_SLOT as in t3_crc_fp4_body.inc.  Workgroup blockIdx.x of its stream, added into the stream's
// accumulator pair.
    __shared__ uint32_t tb[4 * 256 * 4]; __shared__ uint32_t zp[kCrcPows * 32];
    for (int i = threadIdx.x; i < kCrcPows * 32; i += blockDim.x) zp[i] = a.zpow[i];
    __syncthreads();
    {   // T_0[e] = the byte table = "append one zero byte" applied to e; T_{j+1}[e] = T_j[e] advanced by one more zero byte.  (Written as
        // the bit-serial loop, the compiler turned it into loads from a table of its own in global memory, one per bit step.)
        uint32_t c = threadIdx.x;
        for (int j = 0; j < 4; ++j) {
            c = gf2_apply(zp, c);
            for (int cp = 0; cp < 4; ++cp) tb[((j * 256 + threadIdx.x) << 2) + cp] = c;
        }
    }
    __syncthreads();
    const uint32_t ch = blockIdx.x * blockDim.x + threadIdx.x, cp = threadIdx.x & 3u;
    uint32_t sum = 0, part = 0;
    if (ch < a.n_chunks) {
        const uint64_t beg = (uint64_t)ch * a.chunk_bytes, end = min(beg + a.chunk_bytes, a.n_bytes);
        const uint64_t mid = min(beg + (uint64_t)(a.chunk_bytes / 32u) * 16u, end);   // halves start 16-byte aligned
        uint32_t rA = 0, rB = 0;
        uint64_t i = beg, j = mid;
        if (((uintptr_t)T3_CRC_STREAM(a.data) & 15u) == 0) {
            for (; i + 16 <= mid && j + 16 <= end; i += 16, j += 16) {
                const uint4 qa = *(const uint4*)(T3_CRC_STREAM(a.data) + i), qb = *(const uint4*)(T3_CRC_STREAM(a.data) + j);
                const uint32_t wa[4] = {qa.x, qa.y, qa.z, qa.w}, wb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    sum = __builtin_amdgcn_sad_u8(wa[k], 0u, sum); sum = __builtin_amdgcn_sad_u8(wb[k], 0u, sum);
                    rA = crc_word(tb, cp, rA, wa[k]); rB = crc_word(tb, cp, rB, wb[k]);
                }
            }
        }
        for (; i < mid; ++i) { const uint32_t v = T3_CRC_STREAM(a.data)[i]; sum += v; rA = tb[((rA ^ v) & 0xFFu) << 2] ^ (rA >> 8); }
        for (; j < end; ++j) { const uint32_t v = T3_CRC_STREAM(a.data)[j]; sum += v; rB = tb[((rB ^ v) & 0xFFu) << 2] ^ (rB >> 8); }
        const uint32_t r = crc_shift(zp, rA, end - mid) ^ rB;
        part = crc_shift(zp, r, a.n_bytes - end);                    // move it to the end of the stream
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_down(sum, o); part ^= __shfl_down(part, o); }
    if ((threadIdx.x & 63) == 0) { if (part) atomicXor(T3_CRC_SLOT(a.chunk_crc), part); if (sum) atomicAdd(T3_CRC_SLOT(a.sym_sum), sum); }
