// Host replay of the reduced-precision fp32 GETT kernel's tile staging (cudalibrarysamples_amd/csrc/kernels/gett_gen_f32x.inc over the
// index arithmetic of gett_gen_layout.h): for every (planes, tile rows, BK, orientation, vector width) the kernel table instantiates,
// all 256 threads stage their units of V fp32 elements into the 16-bit image(s) exactly as F32xOperand::store does — one 8-byte write of
// four consecutive k (K-contiguous, V = 4), four transposing 2-byte writes (free-contiguous, V = 4), one 2-byte write (V = 1); plane pl
// at pl * ROWS * RB — and every lane of a wave then reads its MFMA fragments exactly as the kernel's compute step does (one 16-byte
// unit per k-block, GenFrag<2>).  Checked: every byte of every plane is written exactly once, 8-byte writes stay inside one 16-byte
// unit and are 8-byte aligned, and the element a lane reads for (plane, k-block s, element e) of row rb + r is element
// (rb + r, GenFrag::k_of(s, q, 0, e)) of that plane.  Test infrastructure (tests/test_f32x_layout_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gett_gen_layout.h"

using namespace ctamd;

static int failures = 0;

template <int PLANES, int ORIENT, int ROWS, int BK, int V>
static void replay(const char* name) {
    using Map = GenUnitMap<ORIENT, ROWS, BK, V, 256>;
    using Img = GenImage<2, BK>;
    using Frag = GenFrag<2>;
    const int planeBytes = ROWS * Img::RB, bytes = PLANES * planeBytes;
    std::vector<int> writes(bytes, 0);
    std::vector<unsigned char> image(bytes, 0);
    // 16-bit element (plane, row, k), byte b, holds a hash of all four
    auto val = [](int pl, int row, int k, int b) { return (unsigned char)((pl * 89 + row * 131 + k * 17 + b * 7 + 3) & 0xff); };
    for (int tid = 0; tid < 256; ++tid) {
        const int kl = Map::unit_k(tid);
        for (int i = 0; i < Map::NU; ++i) {
            const int row = Map::unit_row(tid, i);
            for (int pl = 0; pl < PLANES; ++pl) {
                const int base = pl * planeBytes;
                if (V != 1 && ORIENT == 1) {
                    const int a = Img::addr(row, kl);
                    if ((a & 7) != 0 || ((a & 15) + 8) > 16) { std::printf("%s: the 8-byte write at %d leaves its 16-byte unit\n", name, a); ++failures; return; }
                }
                for (int e = 0; e < V; ++e) {
                    const int er = ORIENT ? row : row + e, ek = ORIENT ? kl + e : kl;
                    const int a = (ORIENT || V == 1) ? Img::addr(row, kl) + e * 2 : Img::addr(row + e, kl);
                    if (er >= ROWS || ek >= BK || a < 0 || a + 2 > planeBytes) { std::printf("%s: unit out of the tile (tid %d unit %d)\n", name, tid, i); ++failures; return; }
                    for (int b = 0; b < 2; ++b) { image[base + a + b] = val(pl, er, ek, b); ++writes[base + a + b]; }
                }
            }
        }
    }
    for (int a = 0; a < bytes; ++a)
        if (writes[a] != 1) { std::printf("%s: byte %d written %d times\n", name, a, writes[a]); ++failures; return; }
    const int KB = BK / Frag::KPB;
    if (KB < 1 || BK % Frag::KPB != 0) { std::printf("%s: BK is not whole k-blocks\n", name); ++failures; return; }
    std::vector<int> kSeen(BK, 0);
    for (int pl = 0; pl < PLANES; ++pl)
        for (int rb = 0; rb < ROWS; rb += 16)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, q = lane >> 4;
                for (int s = 0; s < KB; ++s) {
                    // the kernel: fragOff[s] = unit_addr(0, r, unit(s, q, 0)); address = tile + plane + rb * RB + fragOff
                    const int a = pl * planeBytes + rb * Img::RB + Img::unit_addr(0, r, Frag::unit(s, q, 0));
                    if (a != pl * planeBytes + Img::unit_addr(rb, r, Frag::unit(s, q, 0))) { std::printf("%s: swizzle period broken at rb %d\n", name, rb); ++failures; return; }
                    for (int e = 0; e < Frag::EPU; ++e) {
                        const int k = Frag::k_of(s, q, 0, e);
                        if (pl == 0 && rb == 0 && r == 0) ++kSeen[k];
                        for (int b = 0; b < 2; ++b)
                            if (image[a + e * 2 + b] != val(pl, rb + r, k, b)) {
                                std::printf("%s: plane %d lane %d block %d elem %d of row %d is not (row, k = %d)\n", name, pl, lane, s, e, rb + r, k);
                                ++failures;
                                return;
                            }
                    }
                }
            }
    for (int k = 0; k < BK; ++k)
        if (kSeen[k] != 1) { std::printf("%s: k = %d consumed %d times per row\n", name, k, kSeen[k]); ++failures; return; }
}

// REPLAY(planes, rows, BK, V): both orientations
#define REPLAY(P, ROWS, BK, V) replay<P, 0, ROWS, BK, V>(#P " plane(s) " #ROWS "x" #BK " V" #V " free-contiguous"); \
                               replay<P, 1, ROWS, BK, V>(#P " plane(s) " #ROWS "x" #BK " V" #V " K-contiguous");

int main() {
    // 16BF / 16F: one image per operand
    REPLAY(1, 128, 64, 4) REPLAY(1, 64, 64, 4) REPLAY(1, 128, 32, 1) REPLAY(1, 64, 32, 1)
    // TF32: hi and lo images
    REPLAY(2, 128, 32, 4) REPLAY(2, 64, 32, 4) REPLAY(2, 128, 32, 1) REPLAY(2, 64, 32, 1)
    if (failures) { std::printf("%d layout failures\n", failures); return 1; }
    std::printf("gen f32x layout ok\n");
    return 0;
}
