// Host replay of the tile staging of the single-precision-compute fp64 / complex128 GETT kernel
// (cudalibrarysamples_amd/csrc/kernels/gett_gen_f64x.inc) through the index arithmetic it compiles in (gett_gen_layout.h): for every
// (staged element bytes, BM, BN, BK, V) of its kernel table and each of the four orientation pairs, all 256 threads stage their units of
// the A tile and of the B tile exactly as F64xOperand::store does — a unit is V source elements, each ROUNDED element ES bytes in the
// image — and every lane of a wave then reads its MFMA fragments exactly as the kernel's compute step does.  Checked: every element slot
// of an image is written exactly once; the element a lane feeds to MFMA step j of k-block s is element (row, k) with row = the lane's
// row and k = GenFrag::k_of; every k of the K-tile is consumed exactly once per row; and the A lane and the B lane of the same
// (q, s, step) hold the SAME k.  Test infrastructure (tests/test_f64x_layout_cpu.py).
#include <cstdio>
#include <vector>

#include "gett_gen_layout.h"

using namespace ctamd;

static int failures = 0;

// tag of element (row, k): row * 4096 + k; -1: never written
template <int ES, int ORIENT, int ROWS, int BK, int V>
static bool stage(const char* name, std::vector<int>& tag) {
    using Map = GenUnitMap<ORIENT, ROWS, BK, V, 256>;
    using Img = GenImage<ES, BK>;
    const int bytes = ROWS * Img::RB;
    tag.assign(bytes / ES, -1);
    for (int tid = 0; tid < 256; ++tid) {
        const int kl = Map::unit_k(tid);
        for (int i = 0; i < Map::NU; ++i) {
            const int row = Map::unit_row(tid, i);
            for (int e = 0; e < V; ++e) {
                // the element this unit's e-th slot holds, and where F64xOperand::store puts it: a K-contiguous V = 2 unit is ONE 8-byte
                // write at addr(row, kl) (elements at + 0 and + ES), a free-contiguous one is V writes at addr(row + e, kl)
                const int er = ORIENT ? row : row + e, ek = ORIENT ? kl + e : kl;
                const int a = ORIENT ? Img::addr(row, kl) + e * ES : Img::addr(row + e, kl);
                if (ORIENT && V > 1 && (Img::addr(row, kl) & (V * ES - 1)) != 0) { std::printf("%s: a %d-byte LDS write is not aligned\n", name, V * ES); ++failures; return false; }
                if (er >= ROWS || ek >= BK || a < 0 || a + ES > bytes || a % ES != 0) { std::printf("%s: unit out of the tile (tid %d unit %d)\n", name, tid, i); ++failures; return false; }
                if (tag[a / ES] != -1) { std::printf("%s: slot %d written twice\n", name, a / ES); ++failures; return false; }
                tag[a / ES] = er * 4096 + ek;
            }
        }
    }
    for (size_t s = 0; s < tag.size(); ++s)
        if (tag[s] == -1) { std::printf("%s: slot %zu never written\n", name, s); ++failures; return false; }
    return true;
}

// the (row, k) tag the lane (r, q) of the 16-row block at rb feeds to MFMA step `step` of k-block s, as the kernel's compute step reads
// it: real data (ES = 4) — one unit per lane, element `step`; complex data (ES = 8) — two units per lane, element step & 1 of unit step >> 1
template <int ES, int BK>
static int fragment_tag(const std::vector<int>& tag, int rb, int r, int q, int s, int step, int* kWant) {
    using Img = GenImage<ES, BK>;
    using Frag = GenFrag<ES>;
    const int h = (ES == 4) ? 0 : step >> 1, e = (ES == 4) ? step : step & 1;
    const int a = rb * Img::RB + Img::unit_addr(0, r, Frag::unit(s, q, h)) + e * ES;      // fragOff[s][h] is computed for block 0
    *kWant = Frag::k_of(s, q, h, e);
    return tag[a / ES];
}

template <int ES, int OA, int OB, int BM, int BN, int BK, int V>
static void replay(const char* name) {
    using Frag = GenFrag<ES>;
    static_assert(Frag::UPL * Frag::EPU == 4, "four MFMA steps per k-block");
    std::vector<int> ta, tb;
    if (!stage<ES, OA, BM, BK, V>(name, ta) || !stage<ES, OB, BN, BK, V>(name, tb)) return;
    const int KB = BK / Frag::KPB;
    if (KB < 1 || BK % Frag::KPB != 0) { std::printf("%s: BK is not whole k-blocks\n", name); ++failures; return; }
    std::vector<int> kSeen(BK, 0);
    for (int q = 0; q < 4; ++q)
        for (int s = 0; s < KB; ++s)
            for (int step = 0; step < 4; ++step) {
                int kA = -1, kB = -1;
                for (int rb = 0; rb < BM; rb += 16)
                    for (int r = 0; r < 16; ++r) {
                        const int t = fragment_tag<ES, BK>(ta, rb, r, q, s, step, &kA);
                        if (t != (rb + r) * 4096 + kA) { std::printf("%s: A lane (r %d, q %d) block %d step %d of row %d is not (row, k = %d)\n", name, r, q, s, step, rb + r, kA); ++failures; return; }
                    }
                for (int rb = 0; rb < BN; rb += 16)
                    for (int r = 0; r < 16; ++r) {
                        const int t = fragment_tag<ES, BK>(tb, rb, r, q, s, step, &kB);
                        if (t != (rb + r) * 4096 + kB) { std::printf("%s: B lane (r %d, q %d) block %d step %d of row %d is not (row, k = %d)\n", name, r, q, s, step, rb + r, kB); ++failures; return; }
                    }
                if (kA != kB) { std::printf("%s: A and B disagree on k (q %d block %d step %d: %d vs %d)\n", name, q, s, step, kA, kB); ++failures; return; }
                ++kSeen[kA];
            }
    for (int k = 0; k < BK; ++k)
        if (kSeen[k] != 1) { std::printf("%s: k = %d consumed %d times per row\n", name, k, kSeen[k]); ++failures; return; }
}

#define PAIR(ES, BM, BN, BK, V)                                                       \
    replay<ES, 0, 0, BM, BN, BK, V>(#ES "B " #BM "x" #BN "x" #BK " V" #V " (F, F)");  \
    replay<ES, 0, 1, BM, BN, BK, V>(#ES "B " #BM "x" #BN "x" #BK " V" #V " (F, K)");  \
    replay<ES, 1, 0, BM, BN, BK, V>(#ES "B " #BM "x" #BN "x" #BK " V" #V " (K, F)");  \
    replay<ES, 1, 1, BM, BN, BK, V>(#ES "B " #BM "x" #BN "x" #BK " V" #V " (K, K)");

int main() {
    // fp64 data staged as fp32 (GEN_F64_F32)
    PAIR(4, 128, 128, 32, 2) PAIR(4, 64, 64, 32, 2) PAIR(4, 128, 128, 32, 1) PAIR(4, 64, 64, 32, 1)
    // complex128 data staged as complex64 (GEN_C64_C32)
    PAIR(8, 128, 64, 16, 1) PAIR(8, 64, 64, 16, 1)
    if (failures) { std::printf("%d layout failures\n", failures); return 1; }
    std::printf("f64x layout ok\n");
    return 0;
}
