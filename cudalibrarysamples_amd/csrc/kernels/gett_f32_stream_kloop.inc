// gett_f32_stream_kloop.inc — the multiplying waves of gett_f32_stream_kernel from their first barrier to the last MFMA, included by
// both entries of the kernel (gett_f32_stream.hip), so that the K loop, its barriers and the LDS reads are one text.  Expects in
// scope: Cfg, BM, BN, S, TM, TN, STAGE, OpA, OpB, lds, nTiles, wave, wave8, lane, tlog, lane_now(), stamp(slot); leaves the
// accumulators in acc[TM][TN] and wm / wn (this wave's place in the 2 x 2 wave grid).  Included with CTAMD_KLOOP_EARLY_PARTIALS 1 (the
// flat entries; also expects partials_rsrc()), it stores acc as the slice's partial image as well: nothing is left to the includer.
    // =============================== multipliers ======================================================
    __builtin_amdgcn_s_setprio(2);
    const int wm = wave & 1, wn = wave >> 1;
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int baseA[TM], baseB[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) baseA[i] = OpA::frag_base(wm * (BM / 2) + 16 * i, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) baseB[j] = OpB::frag_base(wn * (BN / 2) + 16 * j, lane);

    f32x4 a0[TM], b0[TN], a1[TM], b1[TN];   // fragments of the even / odd 16-step
    auto load0 = [&](const float* st) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a0[i] = OpA::template fragment<0>(st, baseA[i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) b0[j] = OpB::template fragment<0>(st + OpA::FLOATS, baseB[j]);
    };
    auto load1 = [&](const float* st) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a1[i] = OpA::template fragment<1>(st, baseA[i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) b1[j] = OpB::template fragment<1>(st + OpA::FLOATS, baseB[j]);
    };
    // MFMAs [FIRST, LAST) of one 16-step, numbered kk-major so that consecutive MFMAs never share an
    // accumulator (dependent latency 40 cycles > issue interval 32)
#define CTAMD_MFMA_RANGE(FA, FB, FIRST, LAST)                                                          \
    _Pragma("unroll") for (int kk = 0; kk < 4; ++kk)                                                   \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                   \
        const int idx = (kk * TM + i) * TN + j;                                                        \
        if (Cfg::ABL != 2 && idx >= (FIRST) && idx < (LAST))                                           \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(FA[i][kk], FB[j][kk], acc[i][j], 0, 0, 0); \
    }
    constexpr int NMFMA = 4 * TM * TN;          // MFMAs per 16-step
    constexpr int SPLIT = NMFMA / 3;            // MFMAs of the odd step issued before the barrier
    // scheduling hint: n x (1 MFMA, 1 LDS read)
#define CTAMD_INTERLEAVE_DS(n)                                         \
    _Pragma("unroll") for (int z = 0; z < (n); ++z) {                  \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);             \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);             \
    }

    __builtin_amdgcn_s_barrier();                          // #0: tile 0 has landed
    __builtin_amdgcn_sched_barrier(0);
    load0(lds);
    stamp(1);
    unsigned long long waitC = 0;   // ABL == 3: cycles this wave spent in the per-tile barrier

    // One K-tile in ring slot U (compile-time, so every LDS address is base + immediate).  The fragments
    // of the odd 16-step are fetched under the MFMAs of the even step; the barrier sits a third into the
    // odd step and the first fragments of the next tile are fetched under the remaining two thirds.
#define CTAMD_TILE_BODY(U, LASTTILE) CTAMD_TILE_BODY_AT(lds + (U) * STAGE, lds + (((U) + 1) % S) * STAGE, LASTTILE)
#define CTAMD_TILE_BODY_AT(CUR, NXT, LASTTILE) CTAMD_TILE_BODY_AT2(CUR, NXT, LASTTILE, load0, load1)
#define CTAMD_TILE_BODY_AT2(CUR, NXT, LASTTILE, load0, load1)                                              \
    {                                                                                                      \
        const float* cur = (CUR);                                                                          \
        const float* nxt = (NXT);                                                                          \
        load1(cur);                                                                                        \
        CTAMD_MFMA_RANGE(a0, b0, 0, NMFMA)                                                                 \
        CTAMD_INTERLEAVE_DS(TM + 4 * TN)                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        CTAMD_MFMA_RANGE(a1, b1, 0, SPLIT)                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if constexpr (!(LASTTILE)) {                                                                       \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* this wave's reads of the tile are back */ \
            unsigned long long cb0 = 0;                                                                    \
            if constexpr (Cfg::ABL == 3) cb0 = __builtin_readcyclecounter();                               \
            __builtin_amdgcn_s_barrier();                                                                  \
            if constexpr (Cfg::ABL == 3) waitC += __builtin_readcyclecounter() - cb0;                      \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            load0(nxt);                                                                                    \
            CTAMD_MFMA_RANGE(a1, b1, SPLIT, NMFMA)                                                         \
            CTAMD_INTERLEAVE_DS(TM + 4 * TN)                                                               \
        } else {                                                                                           \
            CTAMD_MFMA_RANGE(a1, b1, SPLIT, NMFMA)                                                         \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    }
#if CTAMD_KLOOP_EARLY_PARTIALS
    // The LAST K-tile of a flat entry (gett_f32_stream_flat_body defines CTAMD_KLOOP_EARLY_PARTIALS 1 and partials_rsrc()), issued by
    // accumulator instead of kk-major, so that the split-K partials leave under its MFMAs and not in one burst behind them.  The
    // fragments go in groups of two (the first group of three when TM x TN is odd); a group's 8 k-steps x its accumulators are issued
    // k-step by k-step, alternating between the accumulators (no two consecutive MFMAs share one), and every accumulator receives
    // 16-step 0 with kk 0..3, then 16-step 1 with kk 0..3 — the kk-major order's own chain, so the bits are the same.  A group that is
    // final is stored under the NEXT group, one 1-KiB store behind each of its first k-steps: the store never waits for the MFMA whose
    // result it reads, and the memory pipe of a multiplying wave, idle until here, takes the tile image while the matrix pipe is busy.
    // Behind the last group only its own two stores remain.  The odd 16-step's fragments are fetched under the first group's MFMAs.
    // Same addresses as the general entry's epilogue: [slice][wave][i][j][lane] x 16 B.
#define CTAMD_TILE_LAST_EARLY(U)                                                                           \
    {                                                                                                      \
        constexpr int NF = TM * TN, G0 = 2 + (NF & 1), NG = (NF - G0) / 2 + 1;                             \
        static_assert(NF >= 4, "at least two groups of fragments");                                        \
        const uint32_t laneBytes = (uint32_t)lane_now() * 16u;                                             \
        const BufRsrc rP = partials_rsrc();                                                                \
        load1(lds + (U) * STAGE);                                                                          \
        _Pragma("unroll") for (int g = 0; g < NG; ++g) {                                                   \
            const int f0 = g == 0 ? 0 : G0 + 2 * (g - 1), nf = g == 0 ? G0 : 2;    /* this group */        \
            const int pf0 = g <= 1 ? 0 : f0 - 2, pnf = g == 0 ? 0 : (g == 1 ? G0 : 2);   /* the one before */ \
            _Pragma("unroll") for (int s = 0; s < 8; ++s) {                                                \
                _Pragma("unroll") for (int c = 0; c < nf; ++c) {                                           \
                    const int i = (f0 + c) / TN, j = (f0 + c) % TN, kk = s & 3;                            \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(s < 4 ? a0[i][kk] : a1[i][kk],        \
                                                                     s < 4 ? b0[j][kk] : b1[j][kk], acc[i][j], 0, 0, 0); \
                }                                                                                          \
                if (s < pnf) {                                                                             \
                    __builtin_amdgcn_sched_barrier(0);                                                     \
                    store_wt_16(acc[(pf0 + s) / TN][(pf0 + s) % TN], rP, (uint32_t)((pf0 + s) * 1024) + laneBytes); \
                    __builtin_amdgcn_sched_barrier(0);                                                     \
                }                                                                                          \
            }                                                                                              \
            if (g == 0) {    /* n x (1 MFMA, 2 LDS reads): the odd step's fragments are back before the group's fifth k-step */ \
                _Pragma("unroll") for (int z = 0; z < (TM + 4 * TN + 1) / 2; ++z) {                        \
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                     \
                }                                                                                          \
            }                                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                             \
        }                                                                                                  \
        stamp(3);                                                                                          \
        _Pragma("unroll") for (int f = NF - 2; f < NF; ++f)                                                \
            store_wt_16(acc[f / TN][f % TN], rP, (uint32_t)(f * 1024) + laneBytes);                        \
    }
#endif
#define CTAMD_BODY_MID(U) CTAMD_TILE_BODY(U, false)
    // compile-time unrolling over the ring slots
#define CTAMD_FOR_SLOTS(M)                                                     \
    { M(0) M(1) M(2)                                                           \
      if constexpr (S > 3) { M(3) } if constexpr (S > 4) { M(4) }              \
      if constexpr (S > 5) { M(5) } }
    // whole ring turns whose S tiles all have a successor, then the last 1 .. S tiles (slots 0 .. r-1)
    int t = 0;
    for (; t + S < nTiles; t += S) CTAMD_FOR_SLOTS(CTAMD_BODY_MID)
    stamp(2);
    const int r = nTiles - t;
#define CTAMD_BODY_END(U) CTAMD_TILE_BODY(U, (U) == S - 1)
#if CTAMD_KLOOP_EARLY_PARTIALS
    // the flat entries: the same three ends, the last tile fragment by fragment with the partials stored under it (stamp(3) is inside)
    static_assert(Cfg::FLAT && S == 3, "the flat entries run the 3-deep ring");
    if (r == S) {
        CTAMD_TILE_BODY(0, false)
        CTAMD_TILE_BODY(1, false)
        CTAMD_TILE_LAST_EARLY(2)
    } else if (r == 2) {
        CTAMD_TILE_BODY(0, false)
        CTAMD_TILE_LAST_EARLY(1)
    } else {
        CTAMD_TILE_LAST_EARLY(0)
    }
#else
    if (r == S) {          // the common case (whole ring turns): straight-line code, no per-tile branch
        CTAMD_FOR_SLOTS(CTAMD_BODY_END)
    } else if constexpr (Cfg::FLAT && CTAMD_FLAT_STRAIGHT_TAIL) {
        // the flat entries (3-deep ring, 96 x 96: registers to spare): one or two tiles left, straight-line code on compile-time slots
        // like the steady loop's — the rolled form below costs ~500 cycles more per tile (run-time slot addresses, fragment bases
        // re-derived per use), and the headline's 32 K-tiles per slice always end in two of them
        static_assert(S == 3, "the flat entries run the 3-deep ring");
        if (r == 2) {
            CTAMD_TILE_BODY(0, false)
            CTAMD_TILE_BODY(1, true)
        } else {
            CTAMD_TILE_BODY(0, true)
        }
    } else {
        // 1 .. S - 1 tiles left (slots 0 .. r - 1): ONE rolled copy of the tile body with run-time slot addresses.  (Unrolled
        // per slot with a branch on r in front of every copy, this tail alone spilled 90-180 VGPRs to scratch memory in the
        // 128 x 128 instantiations — and a kernel that spills is one the next unrelated edit can break.)
        // The fragment bases go through an opaque copy per use, so that derived addresses (base ^ 16, base + slot) are formed
        // where they are needed instead of being carried through the loop in registers it does not have.
        auto opaque = [](int v) { asm volatile("" : "+v"(v)); return v; };
        auto load0t = [&](const float* st) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a0[i] = OpA::template fragment<0>(st, opaque(baseA[i]));
#pragma unroll
            for (int j = 0; j < TN; ++j) b0[j] = OpB::template fragment<0>(st + OpA::FLOATS, opaque(baseB[j]));
        };
        auto load1t = [&](const float* st) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a1[i] = OpA::template fragment<1>(st, opaque(baseA[i]));
#pragma unroll
            for (int j = 0; j < TN; ++j) b1[j] = OpB::template fragment<1>(st + OpA::FLOATS, opaque(baseB[j]));
        };
        int u = 0;
#pragma unroll 1
        for (; u + 1 < r; ++u) CTAMD_TILE_BODY_AT2(lds + u * STAGE, lds + (u + 1) * STAGE, false, load0t, load1t)
        CTAMD_TILE_BODY_AT2(lds + u * STAGE, lds, true, load0t, load1t)     // u == r - 1
    }
    stamp(3);
#endif
    if constexpr (Cfg::ABL == 3) {
        if (tlog != nullptr && wave8 == 0 && lane_now() == 0) tlog[8] = waitC;
    }

