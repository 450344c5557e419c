// t3_crc_fp4_body.inc -- the body of the matrix-core CRC-32 kernels, included by crc_fp4_kernel (t3_crc_fp4.hip: one stream) and
// crc_fp4_frames_kernel (t3_crc_frames.hip: blockIdx.y = one of N equal streams).  `a` is the stream's CrcMArgs.  Text inside the kernels,
// as t3_decode_px_body.inc is: as a function that is handed the argument block by reference -- even one that only adds the frame's
// offset to a pointer -- it changed crc_fp4_kernel's code (profiles/frame_records/notes.md).  What differs between the two kernels
// are two macros the including kernel defines: T3_CRC_STREAM(p), the stream's first byte given frame 0's, and T3_CRC_SLOT(p), the
// stream's accumulator or partials given frame 0's.  One workgroup of four waves, blockIdx.x of its stream; its (xor, sum) goes to
// partials[2 blockIdx.x], [2 blockIdx.x + 1] where there are partials, else into the two accumulators by atomics.
    __shared__ uint32_t red[2 * 16];
    const uint32_t lane = threadIdx.x & 63u, n = lane & 31u, kh = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // The rest behind the last whole round (tail_len < 2048 bytes) belongs to wave 0 of workgroup 0, dispatched first and done long before
    // the streaming waves; the rounds start at workgroup 1.  (Composed at the end of the kernel, the rest was on its critical path.)
    const uint32_t tail_wg = a.tail_len ? 1u : 0u;
    const bool in_tail_wg = blockIdx.x < tail_wg;
    const uint32_t wave_g = (blockIdx.x - tail_wg) * (blockDim.x >> 6) + wave;
    // Which rounds a wave owns.  Strided (stride_waves = W > 0): wave g takes rounds g, g + W, g + 2 W ... -- at any moment the chip reads one
    // moving window of W x kDepth x 2 KiB, the way a streaming copy does; a wave on rounds_per_wave consecutive rounds of its own makes
    // the chip read at 2048 places 90 KB apart, 2 KiB at a time (3.4 TB/s against the 4.5+ a read-only stream reaches).  A column's next
    // chunk is then 2048 W bytes further on: the feedback slice is the host-built "append 2048 W zero bytes" operator (a.afb).
    const uint32_t W = a.stride_waves;
    uint64_t r0, r1, step;                                                          // rounds r0, r0 + step, ... < r1
    if (in_tail_wg) { r0 = r1 = 0; step = 1; }
    else if (W) { r0 = wave_g; r1 = a.n_rounds; step = W; }
    else { r0 = min((uint64_t)wave_g * a.rounds_per_wave, (uint64_t)a.n_rounds); r1 = min(r0 + a.rounds_per_wave, (uint64_t)a.n_rounds); step = 1; }   // a wave past the end runs zero rounds
    const uint64_t pstep = 2048u * step;
    const uint8_t* p = T3_CRC_STREAM(a.data) + r0 * 2048u + 64u * n + 32u * kh;
    const v16f_ zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t f[4] = {0, 0, 0, 0}, sum = 0;
    // Rounds are latency-bound, not arithmetic-bound: with one round of loads in flight per wave a round took ~2,800 cycles (the memory
    // latency under load) against ~600 of arithmetic; kDepth rounds are kept in flight (8 registers each).
    constexpr uint32_t kDepth = T3_CRC_DEPTH;
    uint4 Q[kDepth][2];
    // A streaming wave's first memory instructions are its first kDepth rounds of payload: all workgroups start together, and whatever
    // stands in front of these loads is a stretch in which the chip reads no payload at all.  The operator slices follow them, and no
    // barrier stands between kernel entry and the round loop.
#pragma unroll
    for (uint32_t d = 0; d < kDepth; ++d) { Q[d][0] = make_uint4(0, 0, 0, 0); Q[d][1] = Q[d][0]; if (r0 + d * step < r1) { Q[d][0] = ld16(p + pstep * d); Q[d][1] = ld16(p + pstep * d + 16); } }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t A[9][4];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        const uint4 q = (s == 8 && W) ? *(const uint4*)(a.afb + (size_t)lane * 4u) : *(const uint4*)(a.afrag + ((size_t)s * 64u + lane) * 4u);
        A[s][0] = q.x; A[s][1] = q.y; A[s][2] = q.z; A[s][3] = q.w;
    }
    // Strided form: the wave's last round is known here, and with it the distance from the end of that round to the stream's end,
    // tail_len + 2048 hi bytes with hi = (last_mod - g) mod W < W.  One column per lane of the two table operators (t3_crc.h); the
    // workgroup that takes the rest, and a wave without rounds, keep distance 0 (entry 0 = identity).
    uint32_t dcol_lo = 0, dcol_hi = 0;
    if (W) {
        const bool moves = !in_tail_wg && wave_g < W && r0 < r1;
        const uint32_t hi = moves ? (a.last_mod >= wave_g ? a.last_mod - wave_g : a.last_mod + W - wave_g) : 0u;
        dcol_lo = a.dist_lo[(moves ? a.tail_len : 0u) * 32u + n];
        dcol_hi = a.dist_hi[hi * 32u + n];
    }
    for (uint64_t r = r0; r < r1; r += kDepth * step, p += pstep * kDepth) {
#pragma unroll
        for (uint32_t d = 0; d < kDepth; ++d) {
            if (r + d * step >= r1) break;
            const uint32_t w[8] = {Q[d][0].x, Q[d][0].y, Q[d][0].z, Q[d][0].w, Q[d][1].x, Q[d][1].y, Q[d][1].z, Q[d][1].w};
            if (r + (d + kDepth) * step < r1) { Q[d][0] = ld16(p + pstep * (d + kDepth)); Q[d][1] = ld16(p + pstep * (d + kDepth) + 16); }   // kDepth rounds ahead, in flight from here on
#pragma unroll
            for (int i = 0; i < 8; ++i) sum = __builtin_amdgcn_sad_u8(w[i], 0u, sum);
            parity_nibbles(mfma_round(A, w, mfma4(A[8], f[0], f[1], f[2], f[3], zero)), f);   // running remainder one round step further on, plus this round
        }
    }
    if (in_tail_wg && wave == 0) {
        // The rest as one round of its own that ends at the stream's end: bytes in front of the rest read as zero (they do not move a
        // zero remainder), so after the column alignment below its remainder is in place and needs no shift.  Lane (n, kh) holds round
        // bytes 64 n + 32 kh .. + 31, i.e. rest bytes from lo on; lanes with leading zeros only load nothing.  Byte loads at clamped
        // addresses: all in flight together, none past the stream's end.
        const uint8_t* t = T3_CRC_STREAM(a.data) + ((uint64_t)a.n_rounds << 11);
        const int32_t lo = (int32_t)(64u * n + 32u * kh + a.tail_len) - 2048;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (lo > -32) {
            uint32_t b[32];
#pragma unroll
            for (int32_t i = 0; i < 32; ++i) b[i] = t[max(lo + i, 0)];
#pragma unroll
            for (int32_t i = 0; i < 32; ++i) w[i >> 2] |= (lo + i >= 0 ? b[i] : 0u) << (8 * (i & 3));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) sum = __builtin_amdgcn_sad_u8(w[i], 0u, sum);
        parity_nibbles(mfma_round(A, w, zero), f);
    }
    // Column n's remainder stands at the end of its last chunk, 64 (31 - n) bytes before the end of the wave's region: five masked steps
    // through the "append 64 * 2^b zero bytes" matrices (slices 9..13) bring every column to the region end
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        const uint4 q = *(const uint4*)(a.afrag + ((size_t)(9 + b) * 64u + lane) * 4u);
        const uint32_t Ab[4] = {q.x, q.y, q.z, q.w};
        uint32_t m[4]; parity_nibbles(mfma4(Ab, f[0], f[1], f[2], f[3], zero), m);
        if (((31u - n) >> b) & 1u) { f[0] = m[0]; f[1] = m[1]; f[2] = m[2]; f[3] = m[3]; }
    }
    // This lane's 16 bits -> register bits (accumulator e = 4 g + q of half kh = row (e & 3) + 8 (e >> 2) + 4 kh), then XOR over the
    // columns: the two halves hold disjoint register bits, so one reduction over the whole wave does both
    uint32_t part = 0;
#pragma unroll
    for (uint32_t e = 0; e < 16; ++e) part |= ((f[e >> 2] >> (4u * (e & 3u))) & 1u) << ((e & 3u) + 8u * (e >> 2) + 4u * kh);
    part = wave_xor(part);
    sum = wave_sum(sum);
    if (W) part = wave_apply_col(dcol_hi, wave_apply_col(dcol_lo, part, lane), lane);
    else {
        // blocked form (measurement knob): the distance bit by bit through the "append 2^j zero bytes" operators, staged here so that the
        // strided form pays nothing for them (W is the same for the whole grid: every thread of the workgroup gets here)
        __shared__ uint32_t zp[kCrcPows * 32];
        for (uint32_t e = threadIdx.x; e < (uint32_t)kCrcPows * 32u; e += blockDim.x) zp[e] = a.zpow[e];
        __syncthreads();
        uint64_t rest = in_tail_wg ? 0u : a.n_bytes - r1 * 2048u;
        for (int j = 0; rest; ++j, rest >>= 1) if (rest & 1u) part = wave_apply4(zp + 32 * j, part, lane);
    }
    if (lane == 0) { red[2 * wave] = part; red[2 * wave + 1] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t x = 0, t = 0;
        for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) { x ^= red[2 * w]; t += red[2 * w + 1]; }
        if (a.partials) { T3_CRC_SLOT(a.partials)[2u * blockIdx.x] = x; T3_CRC_SLOT(a.partials)[2u * blockIdx.x + 1u] = t; }
        else { if (x) atomicXor(T3_CRC_SLOT(a.chunk_crc), x); if (t) atomicAdd(T3_CRC_SLOT(a.sym_sum), t); }
    }
