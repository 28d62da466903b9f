// ew_table_layout_harness.cpp — host replay of the mode-table element-wise and reduction kernels' index arithmetic
// (csrc/kernels/ew_table_layout.h, the very functions the kernels of elementwise_table.hip call).  No GPU.
//
//   ew_table_layout_harness FILE...
//
// Each FILE is one plan as tests/test_many_modes_cpu.py wrote it: a header of int64 words — the number of modes n of the problem, then
// for every mode its extent and its element strides in A, D and C (0 where a tensor lacks the mode; for a reduction a reduced mode has
// D stride -1) — followed by the plan's EwTable, byte for byte (ctamdEwTable).  The harness walks the table as its kernel does — every
// tile and every position of the tile kernel in BOTH orders, every element of the gather kernel, every (kept, reduced) pair of the
// reduction — and checks against the header's ground truth that every element of D is produced exactly once and from the right
// offset in A (and C); for the tile kernel also that the element the write side takes from LDS is the one the read side parked there,
// that no two live positions share an LDS slot, and that every slot lies inside the tile kernel's LDS.
// Without arguments it checks one synthetic 40-digit tile table whose outer strides exceed 2^33 by arithmetic alone.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <unordered_map>
#include <vector>

#include "ew_table_layout.h"

using namespace ctamd;

static int fail(const char* file, const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "%s: %s (%lld, %lld)\n", file, what, a, b);
    return 1;
}

// FastDiv as the planner makes it (host/plan_contraction.cpp make_fastdiv)
static FastDiv fastdiv(uint32_t d) {
    FastDiv f{};
    f.d = d;
    if (d < 2) return f;
    uint32_t s = 0;
    while ((1ull << s) < d) ++s;
    f.magic = (uint32_t)(((1ull << (31 + s)) / d) + 1);
    f.shift = s - 1;
    return f;
}

struct Truth {
    std::vector<int64_t> ext, sA, sD, sC;
};
struct Src { int64_t a, c; int seen; };

// D offset -> (A offset, C offset) of every element of D (reductions: of every kept element, A offset of reduced index 0)
static void enumerate_truth(const Truth& t, bool reduction, std::unordered_map<int64_t, Src>& out, std::map<int64_t, int>* redA) {
    const size_t n = t.ext.size();
    std::vector<int64_t> idx(n, 0);
    for (;;) {
        int64_t oA = 0, oD = 0, oC = 0, rA = 0;
        bool base = true;
        for (size_t i = 0; i < n; ++i) {
            const bool red = reduction && t.sD[i] < 0;
            if (red) { rA += idx[i] * t.sA[i]; base = base && idx[i] == 0; continue; }
            oA += idx[i] * t.sA[i]; oD += idx[i] * t.sD[i]; oC += idx[i] * t.sC[i];
        }
        if (base) out[oD] = Src{oA, oC, 0};
        if (redA != nullptr && oD == 0) (*redA)[rA] = 0;
        size_t k = 0;
        while (k < n && ++idx[k] == t.ext[k]) idx[k++] = 0;
        if (k == n) break;
    }
}

static int check_file(const char* file) {
    FILE* f = std::fopen(file, "rb");
    if (f == nullptr) return fail(file, "cannot open");
    int64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1 || n < 0 || n > 64) { std::fclose(f); return fail(file, "bad header"); }
    Truth t;
    for (int64_t i = 0; i < n; ++i) {
        int64_t w[4];
        if (std::fread(w, 8, 4, f) != 4) { std::fclose(f); return fail(file, "short header"); }
        t.ext.push_back(w[0]); t.sA.push_back(w[1]); t.sD.push_back(w[2]); t.sC.push_back(w[3]);
    }
    EwTable tab;
    const size_t got = std::fread(&tab, 1, sizeof(tab), f);
    std::fclose(f);
    if (got != sizeof(tab)) return fail(file, "short table", (long long)got, (long long)sizeof(tab));
    const EwTable* tp = &tab;
    std::unordered_map<int64_t, Src> truth;
    std::map<int64_t, int> redA;
    enumerate_truth(t, tab.kind == EWT_REDUCE, truth, tab.kind == EWT_REDUCE ? &redA : nullptr);
    auto produce = [&](int64_t oA, int64_t oD, int64_t oC) -> int {
        auto it = truth.find(oD);
        if (it == truth.end()) return fail(file, "an offset outside D is written", oD);
        if (it->second.seen++ != 0) return fail(file, "an element of D is produced twice", oD);
        if (it->second.a != oA) return fail(file, "wrong offset in A", it->second.a, oA);
        if (it->second.c != oC) return fail(file, "wrong offset in C", it->second.c, oC);
        return 0;
    };
    if (tab.kind == EWT_TILE) {
        if (tab.tilePos == 0 || tab.nTileA != tab.nTileD) return fail(file, "tile modes");
        const uint32_t posCap = 2048;     // the most positions any element size's tile kernel has slots for is checked by the caller ("lds")
        if (tab.tilePos > posCap) return fail(file, "tile larger than its LDS", tab.tilePos);
        // the tile-relative tables, once — as the kernel builds them
        std::vector<EwtPosA> pa(tab.tilePos);
        std::vector<EwtPosD> pd(tab.tilePos);
        std::vector<int> slotOwner(posCap, -1);
        for (uint32_t r = 0; r < tab.tilePos; ++r) {
            pa[r] = ewt_pos_a(tp, r);
            pd[r] = ewt_pos_d(tp, r);
            const uint32_t slot = ewt_slot(r);
            if (slot >= posCap || slotOwner[slot] >= 0) return fail(file, "two positions share an LDS slot", r, slot);
            slotOwner[slot] = (int)r;
        }
        for (uint32_t r = 0; r < tab.tilePos; ++r) {
            if (pd[r].rankA >= tab.tilePos) return fail(file, "rank in A's order outside the tile", r, pd[r].rankA);
            if (pa[pd[r].rankA].cuts != pd[r].cuts) return fail(file, "the two orders disagree on a position's cut digits", r);
        }
        for (uint32_t tile = 0; tile < tab.total; ++tile) {
            const EwtOrigin o = ewt_tile_origin(tp, tile);
            for (uint32_t r = 0; r < tab.tilePos; ++r) {
                if (!ewt_live(pd[r].cuts, o.live0, o.live1)) continue;
                const EwtPosA& src = pa[pd[r].rankA];                  // what the read side parked in the slot the write side reads
                if (!ewt_live(src.cuts, o.live0, o.live1)) return fail(file, "the write side reads a slot nobody parked", tile, r);
                if (produce(o.oA + (int64_t)src.relA, o.oD + (int64_t)pd[r].relD, o.oC + (int64_t)pd[r].relC)) return 1;
            }
        }
        // consecutive positions of the read order are consecutive addresses of A along its stride-1 mode
        if (tab.tilePos > 1 && pa[1].relA != 1u) return fail(file, "the read order does not start along A's stride-1 mode", pa[1].relA);
        if (tab.tilePos > 1 && pd[1].relD != 1u) return fail(file, "the write order does not start along D's stride-1 mode", pd[1].relD);
    } else if (tab.kind == EWT_GATHER) {
        for (uint32_t i = 0; i < tab.total; ++i) {
            const EwtOffsets o = ewt_offsets(tp, 0u, tab.nEntries, i);
            if (produce(o.oA, o.oD, o.oC)) return 1;
        }
    } else if (tab.kind == EWT_REDUCE) {
        for (uint32_t k = 0; k < tab.total; ++k) {
            const EwtOffsets o = ewt_offsets(tp, 0u, tab.nKept, k);
            if (produce(o.oA, o.oD, o.oC)) return 1;
        }
        // the reduced offsets: each once, over every split
        if ((uint64_t)tab.splitR * tab.redPerSplit < tab.redTotal) return fail(file, "the splits do not cover the reduced range");
        for (uint32_t r = 0; r < tab.redTotal; ++r) {
            const int64_t a = ewt_offsets(tp, tab.nKept, tab.nRed, r).oA;
            auto it = redA.find(a);
            if (it == redA.end()) return fail(file, "a reduced offset outside A's reduced modes", a);
            if (it->second++ != 0) return fail(file, "a reduced element is visited twice", a);
        }
        for (const auto& kv : redA) if (kv.second != 1) return fail(file, "a reduced element is never visited", kv.first);
    } else {
        return fail(file, "unknown table kind", tab.kind);
    }
    for (const auto& kv : truth) if (kv.second.seen != 1) return fail(file, "an element of D is never produced", kv.first);
    return 0;
}

// 40 modes of extent 2: eleven in the tile (A reads them in the opposite order), 29 outside with strides beyond 2^33 in A and in D
static int check_synthetic() {
    static EwTable tab;
    std::memset(&tab, 0, sizeof(tab));
    int64_t sA[40], sD[40], sC[40];
    for (int k = 0; k < 11; ++k) { sD[k] = 1ll << k; sA[k] = 1ll << (10 - k); sC[k] = 3ll << k; }
    for (int k = 11; k < 40; ++k) { sD[k] = 5ll << (k + 20); sA[k] = 3ll << (71 - k); sC[k] = 7ll << (k + 20); }      // 5 * 2^31 .. 5 * 2^59, 3 * 2^60 .. 3 * 2^32
    tab.kind = EWT_TILE;
    tab.nModes = 40;
    tab.nTileA = tab.nTileD = 11;
    tab.tilePos = 2048;
    for (int k = 0; k < 11; ++k) {
        tab.tileD[k].div = fastdiv(2); tab.tileD[k].sD = (uint32_t)sD[k]; tab.tileD[k].sC = (uint32_t)sC[k]; tab.tileD[k].rankA = 1u << (10 - k);
        tab.tileA[k].div = fastdiv(2); tab.tileA[k].sA = 1u << k;                   // A's order: mode 10 first
    }
    tab.nEntries = 29;
    for (int k = 11; k < 40; ++k) {
        EwTableMode& m = tab.mode[k - 11];
        m.div = fastdiv(2); m.sA = sA[k]; m.sD = sD[k]; m.sC = sC[k];
    }
    tab.total = 1u << 29;
    const EwTable* tp = &tab;
    uint64_t x = 88172645463325252ull;
    for (int trial = 0; trial < 200000; ++trial) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint32_t tile = trial == 0 ? (1u << 29) - 1u : (uint32_t)(x >> 20) & ((1u << 29) - 1u), r = (uint32_t)(x & 2047u);
        uint64_t wantA = 0, wantD = 0, wantC = 0;
        for (int k = 0; k < 11; ++k) if ((r >> k) & 1u) { wantA += (uint64_t)sA[k]; wantD += (uint64_t)sD[k]; wantC += (uint64_t)sC[k]; }
        for (int k = 11; k < 40; ++k) if ((tile >> (k - 11)) & 1u) { wantA += (uint64_t)sA[k]; wantD += (uint64_t)sD[k]; wantC += (uint64_t)sC[k]; }
        const EwtOrigin o = ewt_tile_origin(tp, tile);
        const EwtPosD d = ewt_pos_d(tp, r);
        const EwtPosA a = ewt_pos_a(tp, d.rankA);
        if ((uint64_t)(o.oD + (int64_t)d.relD) != wantD) return fail("synthetic", "offset in D", tile, r);
        if ((uint64_t)(o.oC + (int64_t)d.relC) != wantC) return fail("synthetic", "offset in C", tile, r);
        if ((uint64_t)(o.oA + (int64_t)a.relA) != wantA) return fail("synthetic", "offset in A", tile, r);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        if (check_synthetic()) return 1;
        std::printf("ew table layout ok: synthetic\n");
        return 0;
    }
    for (int i = 1; i < argc; ++i)
        if (check_file(argv[i])) return 1;
    std::printf("ew table layout ok: %d tables\n", argc - 1);
    return 0;
}
