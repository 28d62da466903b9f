// gett_gen_rc64.inc — the general MFMA GETT kernel for ONE real fp64 operand times a complex128 one, C and D complex128 (the two mixed
// rows of the contraction type table: R_64F x C_64F -> C_64F and C_64F x R_64F -> C_64F under COMPUTE_DESC_64F, complex double scalars).
//
// The real operand is staged as what it is: 8-byte elements, half the bytes of a complex128 image, and a product is TWO
// v_mfma_f64_16x16x4_f64 into TWO fp64x4 accumulators per 16 x 16 fragment — re += a · b_re, im += a · b_im — where
// gett_gen_kernel<GEN_C64> on a widened copy issues four, two of them against an imaginary part that is identically zero.  No complex
// image of the real operand exists anywhere: not in LDS, not in a temporary.
//
// Skeleton: gett_gen.inc's — 256 threads (2 x 2 waves) on a 64 x 64 output tile, K-tile 8, two LDS stages, the global loads of tile
// t + 1 in flight under the MFMAs of tile t, one barrier per K-tile; rows past the edge clamped, k past the range loaded from a clamped
// address and zeroed on its way into LDS; GenOperand (gett_gen.inc) stages both operands, each with its own element size and width:
//   complex operand  16-byte interleaved (re, im) elements, V = 1, rows of 128 bytes (GenImage<16, 8>), fragment GenFrag<16>:
//                    two units per lane, elements k = 2 q + h
//   real operand     8-byte elements, V = 2 (one 16-byte load) where strides, extents and alignment admit it, else V = 1; rows of 64
//                    bytes (GenImageR64), fragment GenFragR64: ONE 16-byte unit per lane, (a[2 q], a[2 q + 1]) — the same (q, j) -> k
// Swizzle of the real side's 64-byte rows: unit ^ ((row >> 1) & 3) (GenImageR64).  What tools/lds_swizzle_search.py ("rc64" section)
// found over the GF(2)-linear maps of the row's low four bits: the fragment read (one ds_read_b128 per 16-row block: 64 lanes, 64
// distinct units) is CONFLICT-FREE on gfx950's b128 lane groups; the K-contiguous staging writes (ds_write_b128 at V = 2, ds_write_b64 at
// V = 1) are conflict-free; what REMAINS are the transposing ds_write_b64 of a free-contiguous real operand — 16 lanes write 16 or 32
// consecutive rows at one k — 2-way at V = 1 and 4-way at V = 2 (the family's own 64-byte-row swizzle leaves them 4- / 8-way, no swizzle
// 8- / 16-way; four units per row cannot spread them further).  The complex side is GEN_C64's image, as it stands.
// Conjugation: of the complex operand a sign flip of the staged imaginary part, of the real one the identity, of C as in GEN_C64.
// Epilogue and split-K partials (double2 [slice][L][M][N]) are complex128's; launch_gen_splitk_reduce folds them as GEN_C64's.
//
// The view may swap the caller's operands (lanes run along D's contiguous mode), so the real tensor arrives as kernel-A or kernel-B:
// SIDE 0 / 1, each x four orientation pairs x real V in {2, 1}.
#include "gett_gen.inc"

namespace ctamd {

template <int SIDE_, int OA_, int OB_, int VR_>
struct GenRcCfg {
    static constexpr int SIDE = SIDE_, OA = OA_, OB = OB_, VR = VR_;      // SIDE: the real operand — 0 kernel-A, 1 kernel-B; VR: its width
    static constexpr int BM = 64, BN = 64, BK = 8;
    static constexpr int WM = 2, WN = 2, THREADS = 256;
    static constexpr int TM = BM / (WM * 16), TN = BN / (WN * 16);
    static constexpr int ESA = SIDE == 0 ? 8 : 16, ESB = SIDE == 0 ? 16 : 8;
    static constexpr int VA = SIDE == 0 ? VR : 1, VB = SIDE == 0 ? 1 : VR;
    static_assert(SIDE == 0 || SIDE == 1, "one real operand");
};

struct GenRcAcc { f64x4 re, im; };

template <class Cfg>
__global__ void __launch_bounds__(256, 2) gett_gen_rc64_kernel(const GettParams p) {
    constexpr int BM = Cfg::BM, BN = Cfg::BN, BK = Cfg::BK, SIDE = Cfg::SIDE;
    constexpr int WM = Cfg::WM, TM = Cfg::TM, TN = Cfg::TN;
    constexpr int ESA = Cfg::ESA, ESB = Cfg::ESB;
    using ImgR = GenImageR64;
    using ImgC = GenImage<16, BK>;
    using ImgA = std::conditional_t<SIDE == 0, ImgR, ImgC>;
    using ImgB = std::conditional_t<SIDE == 0, ImgC, ImgR>;
    using OpA = GenOperand<ESA, Cfg::OA, BM, BK, Cfg::VA, ImgA>;
    using OpB = GenOperand<ESB, Cfg::OB, BN, BK, Cfg::VB, ImgB>;
    using FragC = GenFrag<16>;
    static_assert(ImgR::BK == BK && ImgR::ES == 8, "the real image is laid out for this K-tile");
    constexpr int STAGE = OpA::LDS_BYTES + OpB::LDS_BYTES;
    static_assert(BK == FragC::KPB && BK == GenFragR64::KPB, "one k-block per K-tile, the same k range on both sides");
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

    const char* A = static_cast<const char*>(p.A) + group_offset<0>(p.gL, l) * (int64_t)ESA;
    const char* B = static_cast<const char*>(p.B) + group_offset<1>(p.gL, l) * (int64_t)ESB;

    OpA ta;
    OpB tb;
    ta.template init_rows<0>(p.gM, m0, tid);
    tb.template init_rows<0>(p.gN, n0, tid);
    // the complex operand's conjugation; the real one's is the identity
    const bool conjA = SIDE == 1 && p.conjA != 0, conjB = SIDE == 0 && p.conjB != 0;

    GenRcAcc acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) { acc[i][j].re = f64x4{0., 0., 0., 0.}; acc[i][j].im = f64x4{0., 0., 0., 0.}; }

    // per-lane byte offsets of the fragment units (the swizzles have a period of 16 rows: valid for every 16-row block)
    const int fragOffR = ImgR::unit_addr(0, r, GenFragR64::unit(0, q, 0));
    int fragOffC[FragC::UPL];
#pragma unroll
    for (int h = 0; h < FragC::UPL; ++h) fragOffC[h] = ImgC::unit_addr(0, r, FragC::unit(0, q, h));

    auto compute = [&](const char* buf) {
        const char* la = buf + (wm * (BM / WM)) * ImgA::RB;
        const char* lb = buf + OpA::LDS_BYTES + (wn * (BN / Cfg::WN)) * ImgB::RB;
        constexpr int TR = SIDE == 0 ? TM : TN, TC = SIDE == 0 ? TN : TM;
        const char* lr = SIDE == 0 ? la : lb;
        const char* lc = SIDE == 0 ? lb : la;
        f64x2 fr[TR];                 // real elements k = 2 q + j
        f64x4 fc[TC];                 // complex elements k = 2 q + h as (re0, im0, re1, im1)
#pragma unroll
        for (int i = 0; i < TR; ++i) fr[i] = *reinterpret_cast<const f64x2*>(lr + 16 * i * ImgR::RB + fragOffR);
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            const f64x2 c0 = *reinterpret_cast<const f64x2*>(lc + 16 * j * ImgC::RB + fragOffC[0]);
            const f64x2 c1 = *reinterpret_cast<const f64x2*>(lc + 16 * j * ImgC::RB + fragOffC[1]);
            fc[j] = f64x4{c0[0], c0[1], c1[0], c1[1]};
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (SIDE == 0) {
                        const double a = fr[i][kk];
                        acc[i][j].re = __builtin_amdgcn_mfma_f64_16x16x4f64(a, fc[j][2 * kk], acc[i][j].re, 0, 0, 0);
                        acc[i][j].im = __builtin_amdgcn_mfma_f64_16x16x4f64(a, fc[j][2 * kk + 1], acc[i][j].im, 0, 0, 0);
                    } else {
                        const double b = fr[j][kk];
                        acc[i][j].re = __builtin_amdgcn_mfma_f64_16x16x4f64(fc[i][2 * kk], b, acc[i][j].re, 0, 0, 0);
                        acc[i][j].im = __builtin_amdgcn_mfma_f64_16x16x4f64(fc[i][2 * kk + 1], b, acc[i][j].im, 0, 0, 0);
                    }
                }
    };

    // ---- main loop: loads of tile t + 1 in flight under the MFMAs of tile t -------------------------------------------------
    const int nTiles = (kEnd > kBegin) ? (int)((kEnd - kBegin + BK - 1) / BK) : 0;
    uint32_t sa[OpA::NU][OpA::DW], sb[OpB::NU][OpB::DW];
    bool oka = false, okb = false;
    if (nTiles > 0) {
        oka = ta.template load<0>(sa, A, p.gK, kBegin, kEnd, tid);
        okb = tb.template load<1>(sb, B, p.gK, kBegin, kEnd, tid);
        ta.template store<SIDE == 1>(sa, oka, conjA, lds, tid);
        tb.template store<SIDE == 0>(sb, okb, conjB, lds + OpA::LDS_BYTES, tid);
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
            ta.template store<SIDE == 1>(sa, oka, conjA, nxt, tid);
            tb.template store<SIDE == 0>(sb, okb, conjB, nxt + OpA::LDS_BYTES, tid);
        }
        __syncthreads();
    }

    // ---- epilogue: complex128's -------------------------------------------------------------------------------------------
    // accumulator register t of a fragment: row gen_acc_row(q, t), column r
    const uint32_t Mtot = p.gM.total, Ntot = p.gN.total;
    const uint32_t mBase = m0 + wm * (BM / WM), nBase = n0 + wn * (BN / Cfg::WN);
    if (p.partial != nullptr) {
        // split-K: double2 partial tiles [slice][L][M][N], GEN_C64's layout (launch_gen_splitk_reduce)
        const size_t tileOff = ((size_t)slice * p.gL.total + l) * (size_t)Mtot * Ntot;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t m = mBase + 16 * i + gen_acc_row<true>(q, t);
                if (m >= Mtot) continue;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const uint32_t n = nBase + 16 * j + r;
                    if (n >= Ntot) continue;
                    const size_t e = tileOff + (size_t)m * Ntot + n;
                    reinterpret_cast<f64x2*>(p.partial)[e] = f64x2{acc[i][j].re[t], acc[i][j].im[t]};
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
    const double alRe = p.alpha64, alIm = p.alphaIm, beRe = p.beta64, beIm = p.betaIm;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t m = mBase + 16 * i + gen_acc_row<true>(q, t);
            if (m >= Mtot) continue;
            int64_t offDm, offCm;
            if (flat) { offDm = (int64_t)m * p.gM.stride[1][0]; offCm = (int64_t)m * p.cStrideM[0]; }
            else group_offset2<1>(p.gM, p.cStrideM, m, offDm, offCm);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (!okN[j]) continue;
                const int64_t oD = offDm + offDn[j], oC = offCm + offCn[j];
                const double re = acc[i][j].re[t], im = acc[i][j].im[t];
                double oRe = alRe * re - alIm * im, oIm = alRe * im + alIm * re;
                if (beRe != 0.0 || beIm != 0.0) {
                    const double* c = static_cast<const double*>(p.C) + 2 * oC;
                    const double cRe = c[0], cIm = p.conjC ? -c[1] : c[1];
                    oRe += beRe * cRe - beIm * cIm;
                    oIm += beRe * cIm + beIm * cRe;
                }
                *reinterpret_cast<f64x2*>(static_cast<double*>(p.D) + 2 * oD) = f64x2{oRe, oIm};
            }
        }
}

// table entry (gett_gen_common.h, CTAMD_GEN_FAMILY_ENTRY) of one instantiation: vec = the real operand's width, variant = its side
#define CTAMD_GEN_RC64_ENTRY(SIDE, OA, OB, VR) \
    {64, 64, 8, 2, 2, 1, OA, OB, 256, 1, 0, 0, &launch_gen_family<gett_gen_rc64_kernel<GenRcCfg<SIDE, OA, OB, VR>>>, 0, 0, GEN_RC64, VR, "gett_gen_rc64_kernel", SIDE},
// the four orientation pairs (LAY_F = 0: free-contiguous, LAY_K = 1: K-contiguous) of one (real side, real width)
#define CTAMD_GEN_RC64_ORIENTS(SIDE, VR)  \
    CTAMD_GEN_RC64_ENTRY(SIDE, 0, 0, VR)  \
    CTAMD_GEN_RC64_ENTRY(SIDE, 0, 1, VR)  \
    CTAMD_GEN_RC64_ENTRY(SIDE, 1, 0, VR)  \
    CTAMD_GEN_RC64_ENTRY(SIDE, 1, 1, VR)

}  // namespace ctamd
