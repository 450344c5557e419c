// t3_decode_px_body.inc — the body of the fused FIXED pixel decoder, included by its two kernels (t3_decode_px.h): decode_fixed_px_kernel
// (one frame; `a` is the kernel's argument block and `args` names it too) and dec_frames_px (a batch of equal frames; `args` is the
// DecFramesArgs, `a` its frame arguments).  Kept as text inside the kernels, not as a function that takes the block by reference: through
// a reference the argument block is copied to registers whole at the kernel's entry (some 70 scalar registers spilled and reloaded inside
// the tile loop; see header_check_wave, t3_decode_wg.h).  In scope: R, RGB, BCN.  What differs between the two kernels: the px_* overloads
// of t3_decode_px.h.  `cur`, `nxt`, `prev` are tickets; `tile` is the ticket's tile inside its frame.
    constexpr uint32_t TCOP = T3_DEC_PX_TCOP, TBASE = kFx2TPx, MT = kFx2ModPx, QCAP = kFx2QCap;
    constexpr uint32_t NW = T3_DEC_PX_THREADS / 128;                                // producer waves = consumer waves
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef T3_DEC_STAMPS
    const uint64_t st_entry = __builtin_amdgcn_s_memtime(); uint64_t st_first = 0;   // kernel entry -> the first tile's input has landed (wave 0)
#endif
    const Tickets tk = tickets_setup(a);                                             // tile tickets, verdict words: t3_decode_wg.h
    tk.first(tid);
    // verdict in this launch: uncorrectable blocks are counted in LDS and the workgroup adds its sum to the launch's counter once, in front of
    // its done count (Tickets::finish).  Written out in both px kernels: as a helper it moved decode_uep_px_kernel's register allocation
    uint32_t* const failp = a.verdict ? (uint32_t*)(lds + kFx2FailWg) : a.fail;
    if (tid == 0) *(uint32_t*)(lds + kFx2FailWg) = 0u;
    stage_constants<TCOP, TBASE, MT>(a, tid, blockDim.x);
    if constexpr (RGB) { if (tid < 82u) *(uint32_t*)(lds + a.dq_off + 4u * tid) = ((const uint32_t*)a.dq)[tid]; }     // yd[244] | cd[84]
    __syncthreads();
#ifdef T3_DEC_STAMPS
    uint64_t st_acc[6] = {0, 0, 0, 0, 0, 0}, st_prev = __builtin_amdgcn_s_memtime(), st_t0 = st_prev, st_rt0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (a.verdict && px_header_wg(args) && wave == 2u * NW - 1u) {                   // the header check, by a wave that starts idle
        uint32_t want = 0;                                                           // word `lane` of hx, picked HERE: see header_check_wave
#pragma unroll
        for (uint32_t q = 0; q < 24; ++q) want = lane == q ? a.hx[q] : want;           // (kernel arguments are not indexed dynamically)
        px_header_check(args, want, lane);
    }
    const uint8_t* body = a.in + a.hdr_syms;
    const uint32_t n_items = 9u * a.nb;
    const uint32_t units_tile = (a.TS / 13u) * 3u;                                  // pixels per tile
    uint32_t cur = blockIdx.x, nxt = tk.next(1u);   // this interval's tile, the next one's

    if (wave < NW) {
        // ---------------- producers: S + E1, two passes of two sets per tile and wave ----------------
        const uint32_t n = lane & 31u, h = lane >> 5;
        // one constant word and one byte offset (of the block in tile 0) per (pass, set) (t3_decode_fx2.h); the constant is made opaque
        // inside the loop, or the compiler unpacks all four ahead of it and spills the pieces (80-VGPR budget)
        Geo geo[2][2]; uint32_t off0[2][2];
        const uint32_t t_off = 26u * a.nb;                                          // from a tile to the next one, in every band
#pragma unroll
        for (uint32_t p = 0; p < 2; ++p) for (uint32_t q = 0; q < 2; ++q) geo[p][q] = fx2_geo<R>(wave * 128u + p * 64u + q * 32u + n, n_items, a.nb, a.div_nb, 0u, off0[p][q]);
        auto has = [&](uint32_t pass, uint32_t set, uint32_t tile) -> bool { Geo g = geo[pass][set]; asm volatile("" : "+v"(g)); return fx2_has_block<R>(g, tile, a.n_tiles, a.nb); };
        // lanes without a block read the first bytes of the body (always there) and ignore them
        auto run_of = [&](uint32_t pass, uint32_t set, uint32_t tile, const uint8_t* fbody) -> Run<BCN> { return load_run<BCN>(a, fbody, has(pass, set, tile) ? off0[pass][set] + tile * t_off + 10u * h : 0u); };
        // the lane's rows of the first AREG steps of the A operand stay in registers: the same 16 bytes in every set
        constexpr uint32_t AREG = BCN ? 0u : T3_DEC_PX_AREG;
        v4i Ak[AREG ? AREG : 1u];
#pragma unroll
        for (uint32_t st = 0; st < AREG; ++st) Ak[st] = *T3_LDS(const v4i, a.af_off + 16u * (64u * st + lane));
        Run<BCN> PA, PB;                                                           // the next pass's two sets, in flight
        PA.w = u32x4{0, 0, 0, 0}; PB.w = PA.w; if constexpr (BCN) { PA.x = 16u << 8; PB.x = PA.x; PA.w4 = 0; PB.w4 = 0; }
        if (cur < px_n_tiles(args)) { PA = run_of(0, 0, px_tile(args, cur), px_body(args, body, cur)); PB = run_of(0, 1, px_tile(args, cur), px_body(args, body, cur)); }
        for (uint32_t k = 0; cur < px_n_tiles(args); ++k) {
            const uint32_t tile = px_tile(args, cur), buf = k & 1u;
            const uint32_t y_off = a.y_off + buf * a.y_stride, q_off = a.q_off + buf * a.q_stride;
            const uint32_t u2 = 2u * mod3_u32(tile * a.nb), toff = tile * t_off;
            uint32_t raw; asm volatile("" : "=v"(raw));                                 // the counter value of lane 0's draw (no merge with a default: a copy would wait for it)
#pragma unroll
            for (uint32_t pass = 0; pass < 2; ++pass) {
                uint32_t LA[4], LB[4];
                run_bytes<BCN>(PA, LA); run_bytes<BCN>(PB, LB);
#ifdef T3_DEC_STAMPS
                if (k == 0u && pass == 0u) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); st_first = __builtin_amdgcn_s_memtime() - st_entry; }
#endif
                // the ticket for the tile after the next one: requested before this pass's loads, read after its work (the file is built
                // without the compiler's atomic optimiser, which would read the counter back at once)
                if (pass == 1u) {
                    // (the previous pass's loads are taken into registers first: vmcnt completes in order, and behind the conditional draw
                    // the compiler's conservative wait for them would cover the draw as well)
                    asm volatile("" : "+v"(LA[0]), "+v"(LA[1]), "+v"(LA[2]), "+v"(LA[3]), "+v"(LB[0]), "+v"(LB[1]), "+v"(LB[2]), "+v"(LB[3]));
                    if (tid == 0u && tk.dyn) raw = tk.request();
                }
                {   // the next pass's input: in flight under this pass (the producers issue no stores, so it is waited for alone)
                    const uint32_t np = pass ^ 1u, nt = pass == 0 ? cur : nxt;              // (a batch: the next tile may belong to another frame)
                    if (nt < px_n_tiles(args)) { PA = run_of(np, 0, px_tile(args, nt), px_body(args, body, nt)); PB = run_of(np, 1, px_tile(args, nt), px_body(args, body, nt)); }
                }
                if (wave * 128u + pass * 64u < n_items) {                             // (wave-uniform) else: nothing left of the tile for this pass
                    Geo gA = geo[pass][0], gB = geo[pass][1]; asm volatile("" : "+v"(gA), "+v"(gB));
                    const Blk bA = fx2_block(gA, off0[pass][0] + toff, fx2_has_block<R>(gA, tile, a.n_tiles, a.nb), u2, y_off);
                    const Blk bB = fx2_block(gB, off0[pass][1] + toff, fx2_has_block<R>(gB, tile, a.n_tiles, a.nb), u2, y_off);
                    const Synd sA = fx2_set<R, TCOP, TBASE, MT, 0, R, AREG>(bA, LA, lane, a.af_off, a.pat_off, Ak);
                    Synd sB; sB.lo = 0; sB.hi = 0;
                    if (wave * 128u + pass * 64u + 32u < n_items) sB = fx2_set<R, TCOP, TBASE, MT, 0, R, AREG>(bB, LB, lane, a.af_off, a.pat_off, Ak);
                    fx2_own_blocks<R>(a.roots, a.fma_off, px_fail(args, failp, cur), sA, sB, bA, bB, (h ? gB : gA) & 0xFFFFu, lane, kFx2Cnt + 4u * buf, q_off, QCAP);
                }
            }
            if (tid == 0u) tk.publish(buf, raw, nxt);
            T3D_STAMP(0);
            barrier_lds();
            T3D_STAMP(1);
            cur = nxt; nxt = tk.next(buf);
        }
        barrier_lds();                                                             // the consumers' last interval
    } else {
        // ---------------- consumers: BM + D5 of the tile the producers finished in the previous interval ----------------
        const uint32_t cw = wave - NW;
        uint32_t prev = 0;
        for (uint32_t k = 0;; ++k) {
            if (k >= 1u) {
                const uint32_t tile = px_tile(args, prev), buf = (k - 1u) & 1u;
                const uint32_t y_off = a.y_off + buf * a.y_stride, q_off = a.q_off + buf * a.q_stride;
                const uint32_t Q = min(*(const uint32_t*)(lds + kFx2Cnt + 4u * buf), QCAP);
                for (uint32_t e0 = cw * 64u; e0 < Q; e0 += 64u * NW) {
                    const uint32_t e = e0 + lane;
                    if (e < Q) {
                        if constexpr (R == 6 && !BCN) fx3_queue_entry(a.roots, a.fma_off, px_fail(args, failp, prev), e, q_off, QCAP, y_off);   // two or three errors in closed form (t3_decode_fx3.h)
                        else fx2_queue_entry<R>(a.roots, a.fma_off, px_fail(args, failp, prev), e, q_off, QCAP, y_off);
                    }
                }
                T3D_STAMP(2);
                consumer_rendezvous<NW>(k, px_fail(args, failp, prev), lane);                            // every patch is in LDS before any wave converts symbols
                if (tid == 64u * NW) *(uint32_t*)(lds + kFx2Cnt + 4u * buf) = 0;         // every consumer has read Q; the producers touch this counter after the barrier
                T3D_STAMP(3);
                const uint64_t unit0 = (uint64_t)tile * units_tile;
                const uint32_t n_here = (uint32_t)min((uint64_t)units_tile, a.n_units > unit0 ? a.n_units - unit0 : 0ull);
                for (uint32_t j = cw * 64u + lane; 4u * j < a.TS / 13u; j += 64u * NW) fx2_pixels12<RGB>(a, j, y_off, unit0, n_here, px_out_off(args, prev));
                T3D_STAMP(4);
            }
            barrier_lds();
            T3D_STAMP(5);
            if (cur >= px_n_tiles(args)) break;                                            // the producers had no tile in this interval: that was their closing barrier
            prev = cur; cur = nxt; nxt = tk.next(k & 1u);
        }
    }
    px_finish(tk, args, tid);
#ifdef T3_DEC_STAMPS
    if ((tid == 0 || tid == 64u * NW) && a.dbg) {
        uint64_t* d = a.dbg + 16ull * blockIdx.x + (tid ? 8 : 0);
        for (int i = 0; i < 6; ++i) d[i] = st_acc[i];
        d[6] = __builtin_amdgcn_s_memtime() - st_t0; d[7] = __builtin_amdgcn_s_memrealtime() - st_rt0;
        if (tid == 0) { d[2] = st_rt0; d[3] = __builtin_amdgcn_s_memrealtime(); d[4] = st_first; }     // producer slots 2, 3: start / end on the 100 MHz clock
    }
#endif
