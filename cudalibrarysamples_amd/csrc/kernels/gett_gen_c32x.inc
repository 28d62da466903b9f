// gett_gen_c32x.inc — complex64 DATA on the 16-bit matrix rate: the reduced-precision compute descriptors of a complex64 contraction.
//
// The complex product is FOUR real products (a_r b_r, a_i b_i, a_r b_i, a_i b_r), each formed as on real data (gett_gen_f32x.inc):
//
//   compute descriptor   each real product x * y                             MFMA per k-block and fragment pair
//   COMPUTE_DESC_16BF    bf16(x) * bf16(y)                                   v_mfma_f32_16x16x32_bf16 x 4
//   COMPUTE_DESC_16F     fp16(x) * fp16(y)  (|x| > 65504 becomes +-inf)      v_mfma_f32_16x16x32_f16  x 4
//   COMPUTE_DESC_TF32    hi_x hi_y + hi_x lo_y + lo_x hi_y                   v_mfma_f32_16x16x32_bf16 x 12
//                        hi = bf16(x), lo = bf16(x - hi)
//
// Structure of gett_gen_f32x_kernel — 256 threads, 2 x 2 waves, every thread stages NU units of V complex64 elements per operand and
// K-tile (V = 2: one 16-byte load, V = 1: 8-byte gathers; LAY_F / LAY_K per operand), two LDS stages, the loads of tile t + 1 in flight
// under the MFMAs of tile t, one barrier per K-tile, rows clamped at the M / N edges, k past the K end zeroed, mixed-radix decode of a
// multi-digit K, xcd_remap — with the de-interleaving and the conversion between the global load and the LDS write: an operand's stage
// is a REAL and an IMAGINARY 16-bit image (GenImage<2, BK>, GenFrag<2>: the searched swizzles of gett_gen_layout.h), each of one plane
// for 16BF / 16F and of two (hi, lo) for TF32; image (part, plane) lies at (part * PLANES + plane) * ROWS * RB.  Conjugation of an
// input is a sign flip of its imaginary parts on the way in (it commutes with every rounding and with the hi / lo split).
//
// Two fp32 accumulators per 16 x 16 fragment: re += a_r b_r + (-a_i) b_i, im += a_r b_i + a_i b_r — the negated imaginary fragment of
// A is one XOR per register (the sign bit of both 16-bit halves), exact in every plane.  Under TF32 the eight small terms of a fragment
// pair go first, then the four hi * hi ones, as in the real kernel.
// Epilogue and split-K are GEN_C32's: D = alpha * acc + beta * op(C) in fp32 complex arithmetic (a real alpha scales the parts, so that an
// infinite sum stays infinite), C never read when beta == 0; float2
// partials [slice][L][M][N] folded by the complex64 branch of launch_gen_splitk_reduce.
//
// Non-finite values under TF32: a part whose bf16 rounding is not finite goes to the LO plane whole, with hi = 0 (Gen16Cvt), so that
// inf * y arrives as lo_x * hi_y with the right sign and the other two terms are 0 * finite.  Two non-finite factors in one product: NaN.
//
// LDS (static, two stages) and registers:  128 x 128 x 32 — 16BF / 16F: 64 KiB, TF32: 128 KiB; 128 accumulator registers, one workgroup
// per CU (__launch_bounds__(256, 1)).  64 x 64 x 32 — 32 / 64 KiB, two workgroups per CU (__launch_bounds__(256, 2)).
#include "gett_gen_common.h"

namespace ctamd {

template <int GE_, int BM_, int BN_, int BK_, int OA_, int OB_, int V_>
struct C32xCfg {
    static constexpr int GE = GE_, BM = BM_, BN = BN_, BK = BK_, OA = OA_, OB = OB_, V = V_;
    static constexpr int WM = 2, WN = 2, THREADS = 256;
    static constexpr int TM = BM / (WM * 16), TN = BN / (WN * 16);
    using Cvt = Gen16Cvt<GE - GEN_C32_BF16>;      // one fp32 part -> the 16-bit pattern(s) of the mode
    static constexpr int PLANES = Cvt::PLANES;
    static constexpr int IMAGES = 2 * PLANES;                         // per operand: (re, im) x planes
    static constexpr int WGS = (BM * BN <= 64 * 64) ? 2 : 1;          // workgroups per CU the registers and the LDS are budgeted for
    static constexpr int LDS_BYTES = 2 * IMAGES * (BM + BN) * BK * 2;  // two stages
    static_assert(BM % 32 == 0 && BN % 32 == 0, "wave sub-tiles are 16-granular");
    static_assert(V == 2 || V == 1, "16-byte loads of two complex64 or 8-byte gathers");
    static_assert(LDS_BYTES * WGS <= 160 * 1024, "LDS of the workgroups that share a CU");
};

// ---------------------------------------------------------------------------------------------
// One operand of the K-tile: global complex64 -> registers -> the (rounded) 16-bit images of its real and imaginary parts.
// ---------------------------------------------------------------------------------------------
template <class Cvt, int ORIENT, int ROWS, int BK, int V>
struct C32xOperand {
    using Map = GenUnitMap<ORIENT, ROWS, BK, V, 256>;
    using Img = GenImage<2, BK>;
    static constexpr int NU = Map::NU;
    static constexpr int PLANES = Cvt::PLANES;
    static constexpr int PLANE_BYTES = ROWS * Img::RB;
    static constexpr int LDS_BYTES = 2 * PLANES * PLANE_BYTES;
    // byte offset of image (part: 0 re / 1 im, plane: 0 hi / 1 lo) inside the operand's stage
    static __device__ __forceinline__ constexpr int image(int part, int plane) { return (part * PLANES + plane) * PLANE_BYTES; }

    int64_t rowOff[NU];      // complex-element offset of each unit's first row in the operand (clamped to a valid row)

    template <int SLOT_R>
    __device__ __forceinline__ void init_rows(const ModeGroup& g, uint32_t row0, int tid) {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            uint32_t r = row0 + (uint32_t)Map::unit_row(tid, i);
            // ORIENT 0: the extent of the fastest free mode is a multiple of V, so a unit is all inside or all outside
            if (r >= g.total) r = g.total - (ORIENT ? 1u : (uint32_t)V);
            rowOff[i] = (g.n <= 1) ? (int64_t)r * g.stride[SLOT_R][0] : group_offset<SLOT_R>(g, r);
        }
    }

    // Issue the loads of the K-tile at k0: st[i] = (re, im) x V.  Returns whether this thread's k lies inside [k0, kEnd) (if not, a
    // clamped valid address was loaded and store() writes zeros).
    template <int SLOT_K>
    __device__ __forceinline__ bool load(float (&st)[NU][2 * V], const float* __restrict__ X, const ModeGroup& gK, uint32_t k0, uint32_t kEnd,
                                         int tid) const {
        const uint32_t k = k0 + (uint32_t)Map::unit_k(tid);
        const bool ok = k < kEnd;
        const uint32_t kc = ok ? k : kEnd - (ORIENT ? (uint32_t)V : 1u);      // K-contiguous units: the K range is a multiple of V
        const int64_t offK = (gK.n <= 1) ? (int64_t)kc * gK.stride[SLOT_K][0] : group_offset<SLOT_K>(gK, kc);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const float* src = X + 2 * (rowOff[i] + offK);
            if constexpr (V == 2) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src);
                st[i][0] = v[0]; st[i][1] = v[1]; st[i][2] = v[2]; st[i][3] = v[3];
            } else {
                const f32x2 v = *reinterpret_cast<const f32x2*>(src);
                st[i][0] = v[0]; st[i][1] = v[1];
            }
        }
        return ok;
    }

    // Registers -> LDS: de-interleave, conjugate, round (split) each part, write image (part, plane)
    __device__ __forceinline__ void store(const float (&st)[NU][2 * V], bool ok, bool conj, char* lds, int tid) const {
        const int kl = Map::unit_k(tid);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            uint16_t h[V][2][PLANES];      // [element][part][plane]
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float re = ok ? st[i][2 * e] : 0.f;
                float im = ok ? st[i][2 * e + 1] : 0.f;
                if (conj) im = -im;
                Cvt::cvt(re, h[e][0]);
                Cvt::cvt(im, h[e][1]);
            }
            const int row = Map::unit_row(tid, i);
#pragma unroll
            for (int part = 0; part < 2; ++part)
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl) {
                    char* base = lds + image(part, pl);
                    if constexpr (V == 1) {
                        *reinterpret_cast<uint16_t*>(base + Img::addr(row, kl)) = h[0][part][pl];
                    } else if constexpr (ORIENT == 1) {
                        // two consecutive k (the first one even) of one row: 4 bytes inside one 16-byte unit of the image
                        *reinterpret_cast<uint32_t*>(base + Img::addr(row, kl)) = (uint32_t)h[0][part][pl] | ((uint32_t)h[1][part][pl] << 16);
                    } else {
                        // free-contiguous unit: V rows at one k — the transposition happens here
#pragma unroll
                        for (int e = 0; e < V; ++e) *reinterpret_cast<uint16_t*>(base + Img::addr(row + e, kl)) = h[e][part][pl];
                    }
                }
        }
    }
};

template <class Cfg>
__global__ void __launch_bounds__(256, Cfg::WGS) gett_gen_c32x_kernel(const GettParams p) {
    constexpr int GE = Cfg::GE, BM = Cfg::BM, BN = Cfg::BN, BK = Cfg::BK, V = Cfg::V;
    constexpr int WM = Cfg::WM, TM = Cfg::TM, TN = Cfg::TN, PLANES = Cfg::PLANES;
    using OpA = C32xOperand<typename Cfg::Cvt, Cfg::OA, BM, BK, V>;
    using OpB = C32xOperand<typename Cfg::Cvt, Cfg::OB, BN, BK, V>;
    using Img = GenImage<2, BK>;
    using Frag = GenFrag<2>;
    constexpr int STAGE = OpA::LDS_BYTES + OpB::LDS_BYTES;
    constexpr int KB = BK / Frag::KPB;      // k-blocks per K-tile
    static_assert(BK % Frag::KPB == 0 && KB >= 1, "whole k-blocks");
    static_assert(2 * STAGE == Cfg::LDS_BYTES, "static LDS");
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
    prefetch_kernarg<(int)sizeof(GettParams)>();

    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 15, q = lane >> 4;

    uint32_t id = xcd_remap(blockIdx.x, p.nBlocks);
    const uint32_t mt = id % p.tilesM; id /= p.tilesM;
    const uint32_t nt = id % p.tilesN; id /= p.tilesN;
    const uint32_t slice = id % p.splitK;
    const uint32_t l = id / p.splitK;
    const uint32_t m0 = mt * BM, n0 = nt * BN;
    const uint32_t kBegin = slice * p.kPerSlice;
    uint32_t kEnd = kBegin + p.kPerSlice;
    if (kEnd > p.gK.total) kEnd = p.gK.total;

    const float* A = static_cast<const float*>(p.A) + 2 * group_offset<0>(p.gL, l);
    const float* B = static_cast<const float*>(p.B) + 2 * group_offset<1>(p.gL, l);

    OpA ta;
    OpB tb;
    ta.template init_rows<0>(p.gM, m0, tid);
    tb.template init_rows<0>(p.gN, n0, tid);
    const bool conjA = p.conjA != 0, conjB = p.conjB != 0;

    f32x4 accRe[TM][TN], accIm[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            accRe[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            accIm[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    // per-lane byte offset of the fragment unit (the swizzle has a period of 16 rows: valid for every 16-row block)
    int fragOff[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) fragOff[s] = Img::unit_addr(0, r, Frag::unit(s, q, 0));

    constexpr bool F16 = GE == GEN_C32_F16;
    // -x in every 16-bit element: the sign bits of both halves of each register
    auto negated = [](const g16x8& a) {
        const u32x4 w = __builtin_bit_cast(u32x4, a) ^ u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        return __builtin_bit_cast(g16x8, w);
    };

    auto compute = [&](const char* buf) {
        const char* la = buf + (wm * (BM / WM)) * Img::RB;
        const char* lb = buf + OpA::LDS_BYTES + (wn * (BN / Cfg::WN)) * Img::RB;
#pragma unroll
        for (int s = 0; s < KB; ++s) {
            g16x8 fb[2][PLANES][TN];      // [part][plane][fragment]
#pragma unroll
            for (int part = 0; part < 2; ++part)
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        fb[part][pl][j] = *reinterpret_cast<const g16x8*>(lb + OpB::image(part, pl) + 16 * j * Img::RB + fragOff[s]);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                g16x8 ar[PLANES], ai[PLANES], an[PLANES];      // a_r, a_i, -a_i
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl) {
                    ar[pl] = *reinterpret_cast<const g16x8*>(la + OpA::image(0, pl) + 16 * i * Img::RB + fragOff[s]);
                    ai[pl] = *reinterpret_cast<const g16x8*>(la + OpA::image(1, pl) + 16 * i * Img::RB + fragOff[s]);
                    an[pl] = negated(ai[pl]);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (PLANES == 2) {      // the small terms first, then hi * hi: all into the same two accumulators
                        accRe[i][j] = gen_mfma16<F16>(an[1], fb[1][0][j], accRe[i][j]);
                        accRe[i][j] = gen_mfma16<F16>(an[0], fb[1][1][j], accRe[i][j]);
                        accRe[i][j] = gen_mfma16<F16>(ar[1], fb[0][0][j], accRe[i][j]);
                        accRe[i][j] = gen_mfma16<F16>(ar[0], fb[0][1][j], accRe[i][j]);
                        accIm[i][j] = gen_mfma16<F16>(ai[1], fb[0][0][j], accIm[i][j]);
                        accIm[i][j] = gen_mfma16<F16>(ai[0], fb[0][1][j], accIm[i][j]);
                        accIm[i][j] = gen_mfma16<F16>(ar[1], fb[1][0][j], accIm[i][j]);
                        accIm[i][j] = gen_mfma16<F16>(ar[0], fb[1][1][j], accIm[i][j]);
                    }
                    accRe[i][j] = gen_mfma16<F16>(an[0], fb[1][0][j], accRe[i][j]);
                    accRe[i][j] = gen_mfma16<F16>(ar[0], fb[0][0][j], accRe[i][j]);
                    accIm[i][j] = gen_mfma16<F16>(ai[0], fb[0][0][j], accIm[i][j]);
                    accIm[i][j] = gen_mfma16<F16>(ar[0], fb[1][0][j], accIm[i][j]);
                }
            }
        }
    };

    // ---- main loop: loads of tile t + 1 in flight under the MFMAs of tile t -------------------------------------------------
    const int nTiles = (kEnd > kBegin) ? (int)((kEnd - kBegin + BK - 1) / BK) : 0;
    float sa[OpA::NU][2 * V], sb[OpB::NU][2 * V];
    bool oka = false, okb = false;
    if (nTiles > 0) {
        oka = ta.template load<0>(sa, A, p.gK, kBegin, kEnd, tid);
        okb = tb.template load<1>(sb, B, p.gK, kBegin, kEnd, tid);
        ta.store(sa, oka, conjA, lds, tid);
        tb.store(sb, okb, conjB, lds + OpA::LDS_BYTES, tid);
    }
    __syncthreads();
    for (int t = 0; t < nTiles; ++t) {
        const bool more = t + 1 < nTiles;
        if (more) {
            oka = ta.template load<0>(sa, A, p.gK, kBegin + (uint32_t)(t + 1) * BK, kEnd, tid);
            okb = tb.template load<1>(sb, B, p.gK, kBegin + (uint32_t)(t + 1) * BK, kEnd, tid);
        }
        compute(lds + (t & 1) * STAGE);
        if (more) {
            char* nxt = lds + ((t + 1) & 1) * STAGE;      // last read by the MFMAs of tile t - 1: every wave is past that barrier
            ta.store(sa, oka, conjA, nxt, tid);
            tb.store(sb, okb, conjB, nxt + OpA::LDS_BYTES, tid);
        }
        __syncthreads();
    }

    // ---- epilogue (fp32 complex, as GEN_C32's) ---------------------------------------------------------------------------------
    // accumulator register t of a fragment: row 4 q + t, column r
    const uint32_t Mtot = p.gM.total, Ntot = p.gN.total;
    const uint32_t mBase = m0 + wm * (BM / WM), nBase = n0 + wn * (BN / Cfg::WN);
    if (p.partial != nullptr) {
        // split-K: float2 partial tiles [slice][L][M][N], folded by launch_gen_splitk_reduce (the complex64 branch)
        const size_t tileOff = ((size_t)slice * p.gL.total + l) * (size_t)Mtot * Ntot;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t m = mBase + 16 * i + gen_acc_row<false>(q, t);
                if (m >= Mtot) continue;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const uint32_t n = nBase + 16 * j + r;
                    if (n >= Ntot) continue;
                    reinterpret_cast<f32x2*>(p.partial)[tileOff + (size_t)m * Ntot + n] = f32x2{accRe[i][j][t], accIm[i][j][t]};
                }
            }
        return;
    }
    int64_t oDl, oCl;
    group_offset2<2>(p.gL, p.cStrideL, l, oDl, oCl);
    const bool flat = p.gM.n <= 1 && p.gN.n <= 1;
    int64_t offDn[TN], offCn[TN];
    bool okN[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const uint32_t n = nBase + 16 * j + r;
        okN[j] = n < Ntot;
        offDn[j] = oDl; offCn[j] = oCl;
        if (okN[j]) {
            int64_t d, c;
            if (flat) { d = (int64_t)n * p.gN.stride[1][0]; c = (int64_t)n * p.cStrideN[0]; }
            else group_offset2<1>(p.gN, p.cStrideN, n, d, c);
            offDn[j] += d; offCn[j] += c;
        }
    }
    const float alRe = (float)p.alpha64, alIm = (float)p.alphaIm, beRe = (float)p.beta64, beIm = (float)p.betaIm;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t m = mBase + 16 * i + gen_acc_row<false>(q, t);
            if (m >= Mtot) continue;
            int64_t offDm, offCm;
            if (flat) { offDm = (int64_t)m * p.gM.stride[1][0]; offCm = (int64_t)m * p.cStrideM[0]; }
            else group_offset2<1>(p.gM, p.cStrideM, m, offDm, offCm);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (!okN[j]) continue;
                const int64_t oD = offDm + offDn[j], oC = offCm + offCn[j];
                const float re = accRe[i][j][t], im = accIm[i][j][t];
                // (a real alpha scales the two parts: no 0 * inf from an imaginary part that is not there)
                float oRe = alRe * re, oIm = alRe * im;
                if (alIm != 0.f) { oRe -= alIm * im; oIm += alIm * re; }
                if (beRe != 0.f || beIm != 0.f) {
                    const float* c = static_cast<const float*>(p.C) + 2 * oC;
                    const float cRe = c[0], cIm = p.conjC ? -c[1] : c[1];
                    oRe += beRe * cRe - beIm * cIm;
                    oIm += beRe * cIm + beIm * cRe;
                }
                *reinterpret_cast<f32x2*>(static_cast<float*>(p.D) + 2 * oD) = f32x2{oRe, oIm};
            }
        }
}

#define CTAMD_C32X_ORIENTS(GE, BM, BN, BK, V) CTAMD_GEN_FAMILY_ORIENTS(gett_gen_c32x_kernel, C32xCfg, GE, BM, BN, BK, V)

}  // namespace ctamd
