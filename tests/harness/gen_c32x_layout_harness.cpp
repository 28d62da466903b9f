// Host replay of the reduced-precision complex64 GETT kernel's tile staging (cudalibrarysamples_amd/csrc/kernels/gett_gen_c32x.inc over
// the index arithmetic of gett_gen_layout.h): for every (planes, tile rows, BK, orientation, vector width) the kernel table instantiates,
// all 256 threads stage their units of V complex64 elements into the 16-bit images exactly as C32xOperand::store does — per image
// (part: re / im, plane: hi / lo) one 4-byte write of two consecutive k (K-contiguous, V = 2), two transposing 2-byte writes
// (free-contiguous, V = 2), one 2-byte write (V = 1); image (part, plane) at (part * PLANES + plane) * ROWS * RB — and every lane of a
// wave then reads its MFMA fragments exactly as the kernel's compute step does (one 16-byte unit per k-block, GenFrag<2>).  Checked:
// every byte of every image of a stage is written exactly once per K-tile, 4-byte writes are 4-byte aligned and stay inside one 16-byte
// unit, and the element a lane reads for (part, plane, k-block s, element e) of row rb + r is element
// (rb + r, GenFrag::k_of(s, q, 0, e)) of that part and plane.  Test infrastructure (tests/test_c32x_layout_cpu.py).
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
    const int planeBytes = ROWS * Img::RB, images = 2 * PLANES, bytes = images * planeBytes;
    auto image_of = [&](int part, int pl) { return (part * PLANES + pl) * planeBytes; };      // C32xOperand::image
    std::vector<int> writes(bytes, 0);
    std::vector<unsigned char> image(bytes, 0);
    // 16-bit element (part, plane, row, k), byte b, holds a hash of all five
    auto val = [](int part, int pl, int row, int k, int b) { return (unsigned char)((part * 53 + pl * 89 + row * 131 + k * 17 + b * 7 + 3) & 0xff); };
    for (int tid = 0; tid < 256; ++tid) {
        const int kl = Map::unit_k(tid);
        for (int i = 0; i < Map::NU; ++i) {
            const int row = Map::unit_row(tid, i);
            for (int part = 0; part < 2; ++part)
                for (int pl = 0; pl < PLANES; ++pl) {
                    const int base = image_of(part, pl);
                    if (V != 1 && ORIENT == 1) {
                        const int a = Img::addr(row, kl);
                        if ((a & 3) != 0 || ((a & 15) + 4) > 16) { std::printf("%s: the 4-byte write at %d is misaligned or leaves its 16-byte unit\n", name, a); ++failures; return; }
                    }
                    for (int e = 0; e < V; ++e) {
                        const int er = ORIENT ? row : row + e, ek = ORIENT ? kl + e : kl;
                        const int a = (ORIENT || V == 1) ? Img::addr(row, kl) + e * 2 : Img::addr(row + e, kl);
                        if (er >= ROWS || ek >= BK || a < 0 || a + 2 > planeBytes) { std::printf("%s: unit out of the tile (tid %d unit %d)\n", name, tid, i); ++failures; return; }
                        if (ORIENT && V != 1 && a != Img::addr(er, ek)) { std::printf("%s: the second k of a pair is not next to the first (tid %d unit %d)\n", name, tid, i); ++failures; return; }
                        for (int b = 0; b < 2; ++b) { image[base + a + b] = val(part, pl, er, ek, b); ++writes[base + a + b]; }
                    }
                }
        }
    }
    for (int a = 0; a < bytes; ++a)
        if (writes[a] != 1) { std::printf("%s: byte %d written %d times\n", name, a, writes[a]); ++failures; return; }
    const int KB = BK / Frag::KPB;
    if (KB < 1 || BK % Frag::KPB != 0) { std::printf("%s: BK is not whole k-blocks\n", name); ++failures; return; }
    std::vector<int> kSeen(BK, 0);
    for (int part = 0; part < 2; ++part)
        for (int pl = 0; pl < PLANES; ++pl)
            for (int rb = 0; rb < ROWS; rb += 16)
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = lane & 15, q = lane >> 4;
                    for (int s = 0; s < KB; ++s) {
                        // the kernel: fragOff[s] = unit_addr(0, r, unit(s, q, 0)); address = tile + image + rb * RB + fragOff
                        const int a = image_of(part, pl) + rb * Img::RB + Img::unit_addr(0, r, Frag::unit(s, q, 0));
                        if (a != image_of(part, pl) + Img::unit_addr(rb, r, Frag::unit(s, q, 0))) { std::printf("%s: swizzle period broken at rb %d\n", name, rb); ++failures; return; }
                        for (int e = 0; e < Frag::EPU; ++e) {
                            const int k = Frag::k_of(s, q, 0, e);
                            if (part == 0 && pl == 0 && rb == 0 && r == 0) ++kSeen[k];
                            for (int b = 0; b < 2; ++b)
                                if (image[a + e * 2 + b] != val(part, pl, rb + r, k, b)) {
                                    std::printf("%s: part %d plane %d lane %d block %d elem %d of row %d is not (row, k = %d)\n", name, part, pl, lane, s, e, rb + r, k);
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
    // 16BF / 16F: a real and an imaginary image per operand
    REPLAY(1, 128, 32, 2) REPLAY(1, 64, 32, 2) REPLAY(1, 128, 32, 1) REPLAY(1, 64, 32, 1)
    // TF32: re-hi, re-lo, im-hi, im-lo
    REPLAY(2, 128, 32, 2) REPLAY(2, 64, 32, 2) REPLAY(2, 128, 32, 1) REPLAY(2, 64, 32, 1)
    if (failures) { std::printf("%d layout failures\n", failures); return 1; }
    std::printf("gen c32x layout ok\n");
    return 0;
}
