// gett_f32_stream_ring.inc — the data-moving waves' ring schedule of gett_f32_stream_kernel, included by both of its entries
// (gett_f32_stream.hip: the general one and the flat one), so that the order and count of tile requests, the counted waits and the
// barriers are one text.  Expects in scope: Cfg, S, LOADS, nTiles, tid, tlog, issue(slot) — requests the next K-tile into ring
// slot `slot` and advances the odometer — and fix_last() (RAG: repairs the masked last tile; a no-op otherwise).
        if (tlog != nullptr && tid == 256) tlog[7] = __builtin_readcyclecounter();   // setup done, first issue
        // Progressive start: the multiplying waves are released as soon as tile 0 has landed, while the
        // rest of the ring is still being requested (an LDS-DMA issue that misses the TLB takes hundreds
        // of cycles, so S tiles of issue time in front of barrier #0 would be S times the start-up cost).
        issue(0);
        if (nTiles > 1) {
            issue(1);
            CTAMD_WAIT_VMCNT(LOADS);
        } else {
            CTAMD_WAIT_VMCNT(0);
            fix_last();                                    // ONE tile: it is the masked one
        }
        __builtin_amdgcn_s_barrier();                      // #0
#pragma unroll
        for (int T = 2; T < S; ++T)
            if (T < nTiles) issue(T);
        int slot = 0, t = 0;
        unsigned long long waitV = 0, waitB = 0;
        for (; t + S < nTiles; ++t) {                      // outstanding: tiles t+1 .. t+S-1
            unsigned long long c0 = 0, c1 = 0, c2 = 0;
            if constexpr (Cfg::ABL == 3) c0 = __builtin_readcyclecounter();
            if constexpr (Cfg::ABL == 1) CTAMD_WAIT_VMCNT(0); else CTAMD_WAIT_VMCNT(LOADS * (S - 2));
            if constexpr (Cfg::ABL == 3) c1 = __builtin_readcyclecounter();
            __builtin_amdgcn_s_barrier();                  // #(t+1): slot t % S is free
            if constexpr (Cfg::ABL == 3) { c2 = __builtin_readcyclecounter(); waitV += c1 - c0; waitB += c2 - c1; }
            if constexpr (Cfg::ABL != 1) issue(slot);
            slot = (slot + 1 == S) ? 0 : slot + 1;
        }
        if constexpr (Cfg::ABL == 3) {
            if (tlog != nullptr && tid == 256) { tlog[9] = waitV; tlog[10] = waitB; }
        }
        // every tile is on its way: one barrier per remaining tile, waiting for exactly the tiles behind it
        for (; t + 1 < nTiles; ++t) {
            const int behind = nTiles - t - 2;             // tiles issued after tile t+1: 0 .. S-2
            if (behind <= 0) { CTAMD_WAIT_VMCNT(0); fix_last(); }   // tile t + 1 is the last one
            else if (behind == 1) CTAMD_WAIT_VMCNT(LOADS);
            else if (behind == 2) CTAMD_WAIT_VMCNT(LOADS * 2);
            else if (behind == 3) CTAMD_WAIT_VMCNT((S > 4 ? LOADS * 3 : 0));
            else CTAMD_WAIT_VMCNT((S > 5 ? LOADS * 4 : 0));
            __builtin_amdgcn_s_barrier();                  // #(t+1)
        }
        CTAMD_WAIT_VMCNT(0);
        return;
