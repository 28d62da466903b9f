// Host replay of the tile staging of the mixed fp64 x complex128 GETT kernel (cudalibrarysamples_amd/csrc/kernels/gett_gen_rc64.inc) on
// the index arithmetic it compiles in (gett_gen_layout.h): for every (real side, orientation pair, real vector width) of its table, all
// 256 threads stage a 64 x 8 tile of EACH operand exactly as GenOperand::store does — the real one as 8-byte elements in 64-byte rows
// (GenImageR64, units of V doubles), the complex one as 16-byte elements in 128-byte rows (GenImage<16, 8>, single elements) — and
// every lane of a wave then reads its fragments exactly as the kernel's compute step does: ONE 16-byte unit of the real image
// (GenFragR64), two of the complex one (GenFrag<16>).  Checked: every byte of both images is written exactly once; the two-MFMA step j of
// lane (r, q) gets real element (row, k) and complex element (row', k') with k == k' == 2 q + j — both sides agree on k; every k of
// the K-tile is consumed exactly once per row.  Test infrastructure (tests/test_rc64_layout_cpu.py).
#include <cstdio>
#include <vector>

#include "gett_gen_layout.h"

using namespace ctamd;

static int failures = 0;
static const int ROWS = 64, BK = 8;

static unsigned char val(int side, int row, int k, int b) { return (unsigned char)((side * 71 + row * 131 + k * 17 + b * 7 + 3) & 0xff); }

// stage one operand's tile as GenOperand<ES, ORIENT, 64, 8, V>::store does; false: a byte written twice / never / out of the tile
template <class Img, int ORIENT, int V>
static bool stage(const char* name, int side, std::vector<unsigned char>& image) {
    using Map = GenUnitMap<ORIENT, ROWS, BK, V, 256>;
    constexpr int ES = Img::ES;
    const int bytes = ROWS * Img::RB;
    std::vector<int> writes(bytes, 0);
    image.assign(bytes, 0);
    for (int tid = 0; tid < 256; ++tid) {
        const int kl = Map::unit_k(tid);
        for (int i = 0; i < Map::NU; ++i) {
            const int row = Map::unit_row(tid, i);
            for (int e = 0; e < V; ++e) {
                const int er = ORIENT ? row : row + e, ek = ORIENT ? kl + e : kl;
                const int a = (ORIENT || V == 1) ? Img::addr(row, kl) + e * ES : Img::addr(row + e, kl);
                if (er >= ROWS || ek >= BK || a < 0 || a + ES > bytes) { std::printf("%s: unit out of the tile (tid %d unit %d)\n", name, tid, i); return false; }
                for (int b = 0; b < ES; ++b) { image[a + b] = val(side, er, ek, b); ++writes[a + b]; }
            }
        }
    }
    for (int a = 0; a < bytes; ++a)
        if (writes[a] != 1) { std::printf("%s: byte %d of the %d-byte-element image written %d times\n", name, a, ES, writes[a]); return false; }
    return true;
}

// SIDE: the real operand is kernel-A (0) or kernel-B (1); OA / OB: orientations of kernel-A / kernel-B; VR: the real operand's width
template <int SIDE, int OA, int OB, int VR>
static void replay(const char* name) {
    constexpr int OR = SIDE == 0 ? OA : OB, OC = SIDE == 0 ? OB : OA;
    using ImgR = GenImageR64;
    using ImgC = GenImage<16, BK>;
    using FragC = GenFrag<16>;
    std::vector<unsigned char> real, cplx;
    if (!stage<ImgR, OR, VR>(name, 0, real) || !stage<ImgC, OC, 1>(name, 1, cplx)) { ++failures; return; }
    if (GenFragR64::KPB != BK || FragC::KPB != BK) { std::printf("%s: the K-tile is not one k-block on both sides\n", name); ++failures; return; }
    std::vector<int> kSeen(BK, 0);
    for (int rb = 0; rb < ROWS; rb += 16)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 15, q = lane >> 4;
            // the kernel: fragOffR = ImgR::unit_addr(0, r, GenFragR64::unit(0, q, 0)), fragOffC[h] = ImgC::unit_addr(0, r, FragC::unit(0, q, h))
            const int ar = rb * ImgR::RB + ImgR::unit_addr(0, r, GenFragR64::unit(0, q, 0));
            if (ar != ImgR::unit_addr(rb, r, GenFragR64::unit(0, q, 0))) { std::printf("%s: swizzle period broken at rb %d (real)\n", name, rb); ++failures; return; }
            for (int j = 0; j < 2; ++j) {      // MFMA step kk = j: fr[..][j] against fc[..][2 j], fc[..][2 j + 1]
                const int kr = GenFragR64::k_of(0, q, 0, j), kc = FragC::k_of(0, q, j, 0);
                if (kr != kc || kr != 2 * q + j) { std::printf("%s: lane %d step %d: real k = %d, complex k = %d\n", name, lane, j, kr, kc); ++failures; return; }
                if (rb == 0 && r == 0) ++kSeen[kr];
                const int ac = rb * ImgC::RB + ImgC::unit_addr(0, r, FragC::unit(0, q, j));
                if (ac != ImgC::unit_addr(rb, r, FragC::unit(0, q, j))) { std::printf("%s: swizzle period broken at rb %d (complex)\n", name, rb); ++failures; return; }
                for (int b = 0; b < 8; ++b)
                    if (real[ar + 8 * j + b] != val(0, rb + r, kr, b)) {
                        std::printf("%s: lane %d step %d: the real element of row %d is not (row, k = %d)\n", name, lane, j, rb + r, kr);
                        ++failures;
                        return;
                    }
                for (int b = 0; b < 16; ++b)      // bytes 0..7: re, 8..15: im
                    if (cplx[ac + b] != val(1, rb + r, kc, b)) {
                        std::printf("%s: lane %d step %d: the complex element of row %d is not (row, k = %d)\n", name, lane, j, rb + r, kc);
                        ++failures;
                        return;
                    }
            }
        }
    for (int k = 0; k < BK; ++k)
        if (kSeen[k] != 1) { std::printf("%s: k = %d consumed %d times per row\n", name, k, kSeen[k]); ++failures; return; }
}

#define REPLAY_ENTRY(SIDE, OA, OB, VR) replay<SIDE, OA, OB, VR>("side " #SIDE " orient " #OA #OB " V" #VR);
// the four orientation pairs of one (real side, real width): CTAMD_GEN_RC64_ORIENTS of gett_gen_rc64.hip
#define REPLAY_ORIENTS(SIDE, VR) REPLAY_ENTRY(SIDE, 0, 0, VR) REPLAY_ENTRY(SIDE, 0, 1, VR) REPLAY_ENTRY(SIDE, 1, 0, VR) REPLAY_ENTRY(SIDE, 1, 1, VR)

int main() {
    REPLAY_ORIENTS(0, 2) REPLAY_ORIENTS(0, 1) REPLAY_ORIENTS(1, 2) REPLAY_ORIENTS(1, 1)
    if (failures) { std::printf("%d layout failures\n", failures); return 1; }
    std::printf("rc64 layout ok\n");
    return 0;
}
