// gett_gen_f64x.inc — fp64 / complex128 DATA on the fp32 matrix rate: COMPUTE_DESC_32F on a contraction whose tensors are all real
// fp64 or all complex128.
//
//   element        data        staged as                        MFMA per k-block and fragment pair       accumulators per fragment
//   GEN_F64_F32    fp64        fp32, 4-byte image  (ES = 4)     v_mfma_f32_16x16x4_f32 x 4               1 x fp32x4
//   GEN_C64_C32    complex128  complex64, 8-byte image (ES = 8) v_mfma_f32_16x16x4_f32 x 4 per k         3 x fp32x4 (Re·Re, Im·Im, Re·Im + Im·Re)
//
// D = alpha * sum_k fp32(a_k) * fp32(b_k) + beta * op(C): every operand element is rounded ONCE to fp32 (v_cvt_f32_f64: to nearest even,
// |x| >= 2^128 (1 - 2^-25) becomes +-inf, NaN stays NaN; complex data: both parts) between the global load and the LDS write; products
// and sums run on the fp32 MFMA; the epilogue widens the accumulators to double (complex: Re = (double)rr - (double)ii) and applies
// alpha and beta in fp64 on fp64 C / D.  The structure is that of gett_gen_f32x.inc — 256 threads, 2 x 2 waves, every thread stages NU
// units per operand and K-tile (real: V fp64 elements, V = 2: one 16-byte load, V = 1: 8-byte gathers; complex: one element = one
// 16-byte load; LAY_F / LAY_K per operand), two LDS stages, the loads of tile t + 1 in flight under the MFMAs of tile t, one barrier per
// K-tile, rows clamped at the M / N edges, k past the K end zeroed, mixed-radix decode of a multi-digit K, xcd_remap.  Split-K partials
// are fp32 (complex: float2 (Re, Im)) tiles [slice][L][M][N] — half the workspace of the fp64 kernels — folded in fp64 by
// launch_gen_splitk_reduce.  Conjugation of a complex input is a sign flip on the staged imaginary parts; conjC applies in the epilogue.
//
// LDS (gett_gen_layout.h): real data GenImage<4, 32> / GenFrag<4> — 128-byte rows, a lane reads ONE 16-byte unit (k = 4 q .. 4 q + 3 of
// row r) and feeds element j to MFMA step j: the read pattern of the 16-bit image, and its swizzle; complex data the 8-byte image of
// complex64 (GenImage<8, 16> / GenFrag<8>).  Static, two stages: 128 x 128 x 32 real 64 KiB, 128 x 64 x 16 complex 48 KiB.
#include "gett_gen_common.h"

namespace ctamd {

template <int GE_, int BM_, int BN_, int BK_, int OA_, int OB_, int V_>
struct F64xCfg {
    static constexpr int GE = GE_, BM = BM_, BN = BN_, BK = BK_, OA = OA_, OB = OB_, V = V_;
    static constexpr bool CPLX = GE == GEN_C64_C32;
    static constexpr int WM = 2, WN = 2, THREADS = 256;
    static constexpr int TM = BM / (WM * 16), TN = BN / (WN * 16);
    static constexpr int ES = CPLX ? 8 : 4;      // bytes of a STAGED element
    static_assert(GE == GEN_F64_F32 || GE == GEN_C64_C32, "fp64 or complex128 data");
    static_assert(BM % 32 == 0 && BN % 32 == 0, "wave sub-tiles are 16-granular");
    static_assert(CPLX ? V == 1 : (V == 2 || V == 1), "16-byte loads (two fp64 / one complex128) or 8-byte gathers");
};

// ---------------------------------------------------------------------------------------------
// One operand of the K-tile: global fp64 -> registers -> (rounded) fp32 LDS image.
// ---------------------------------------------------------------------------------------------
template <bool CPLX, int ORIENT, int ROWS, int BK, int V>
struct F64xOperand {
    using Map = GenUnitMap<ORIENT, ROWS, BK, V, 256>;
    using Img = GenImage<CPLX ? 8 : 4, BK>;
    static constexpr int NU = Map::NU;
    static constexpr int SD = CPLX ? 2 : 1;      // doubles per source element
    static constexpr int ND = V * SD;            // doubles per unit = per global load: 2 (16 bytes) or 1
    static constexpr int LDS_BYTES = ROWS * Img::RB;
    // Sixteen units per thread (the 128-row tile on 8-byte gathers): sixteen 64-bit row offsets per operand beside sixteen staged doubles
    // and the 128 x 128 accumulators do not fit 256 registers.  Such a thread keeps its (clamped) ROW INDICES, 32 bits each, and turns
    // them into offsets at each load: one 64-bit multiply-add for a fused row group, the mixed-radix decode otherwise.
    static constexpr bool LAZY = NU > 8;
    using RowT = typename std::conditional<LAZY, uint32_t, int64_t>::type;

    RowT rowOff[NU];         // element offset of each unit's first row in the operand (clamped to a valid row) — LAZY: the row itself

    template <int SLOT_R>
    static __device__ __forceinline__ int64_t row_offset(const ModeGroup& g, uint32_t r) {
        return (g.n <= 1) ? (int64_t)r * g.stride[SLOT_R][0] : group_offset<SLOT_R>(g, r);
    }

    template <int SLOT_R>
    __device__ __forceinline__ void init_rows(const ModeGroup& g, uint32_t row0, int tid) {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            uint32_t r = row0 + (uint32_t)Map::unit_row(tid, i);
            // ORIENT 0: the extent of the fastest free mode is a multiple of V, so a unit is all inside or all outside
            if (r >= g.total) r = g.total - (ORIENT ? 1u : (uint32_t)V);
            if constexpr (LAZY) rowOff[i] = r;
            else                rowOff[i] = row_offset<SLOT_R>(g, r);
        }
    }

    // Issue the loads of the K-tile at k0.  Returns whether this thread's k lies inside [k0, kEnd) (if not, a clamped valid
    // address was loaded and store() writes zeros).
    template <int SLOT_R, int SLOT_K>
    __device__ __forceinline__ bool load(double (&st)[NU][ND], const double* __restrict__ X, const ModeGroup& gR, const ModeGroup& gK, uint32_t k0,
                                         uint32_t kEnd, int tid) const {
        const uint32_t k = k0 + (uint32_t)Map::unit_k(tid);
        const bool ok = k < kEnd;
        const uint32_t kc = ok ? k : kEnd - (ORIENT ? (uint32_t)V : 1u);      // K-contiguous units: the K range is a multiple of V
        const int64_t offK = (gK.n <= 1) ? (int64_t)kc * gK.stride[SLOT_K][0] : group_offset<SLOT_K>(gK, kc);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            int64_t offR;
            if constexpr (LAZY) {
                uint32_t row = rowOff[i];
                asm volatile("" : "+v"(row));      // opaque: or the sixteen offsets are hoisted out of the K loop, back into registers
                offR = row_offset<SLOT_R>(gR, row);
            } else {
                offR = rowOff[i];
            }
            const double* src = X + (offR + offK) * (int64_t)SD;
            if constexpr (ND == 2) {
                const f64x2 v = *reinterpret_cast<const f64x2*>(src);
                st[i][0] = v[0]; st[i][1] = v[1];
            } else {
                st[i][0] = *src;
            }
        }
        return ok;
    }

    // Registers -> LDS: round each double to fp32 (the one rounding of the mode).  conj (complex data): flip the sign of the imaginary part.
    __device__ __forceinline__ void store(const double (&st)[NU][ND], bool ok, bool conj, char* lds, int tid) const {
        const int kl = Map::unit_k(tid);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            float f[ND];
#pragma unroll
            for (int d = 0; d < ND; ++d) f[d] = ok ? (float)st[i][d] : 0.f;
            const int row = Map::unit_row(tid, i);
            if constexpr (CPLX) {
                if (conj) f[1] = -f[1];
                *reinterpret_cast<f32x2*>(lds + Img::addr(row, kl)) = f32x2{f[0], f[1]};
            } else if constexpr (V == 1) {
                *reinterpret_cast<float*>(lds + Img::addr(row, kl)) = f[0];
            } else if constexpr (ORIENT == 1) {
                // two consecutive k of one row: 8 bytes inside one 16-byte unit of the image
                *reinterpret_cast<f32x2*>(lds + Img::addr(row, kl)) = f32x2{f[0], f[1]};
            } else {
                // free-contiguous unit: V rows at one k — the transposition happens here
#pragma unroll
                for (int e = 0; e < V; ++e) *reinterpret_cast<float*>(lds + Img::addr(row + e, kl)) = f[e];
            }
        }
    }
};

template <bool CPLX> struct F64xAcc;
template <> struct F64xAcc<false> { f32x4 v; };
template <> struct F64xAcc<true>  { f32x4 rr, ii, x; };

template <class Cfg>
__global__ void __launch_bounds__(256, 2) gett_gen_f64x_kernel(const GettParams p) {
    constexpr int BM = Cfg::BM, BN = Cfg::BN, BK = Cfg::BK, V = Cfg::V;
    constexpr int WM = Cfg::WM, TM = Cfg::TM, TN = Cfg::TN;
    constexpr bool CPLX = Cfg::CPLX;
    constexpr int SD = CPLX ? 2 : 1;
    using OpA = F64xOperand<CPLX, Cfg::OA, BM, BK, V>;
    using OpB = F64xOperand<CPLX, Cfg::OB, BN, BK, V>;
    using Img = GenImage<Cfg::ES, BK>;
    using Frag = GenFrag<Cfg::ES>;
    constexpr int STAGE = OpA::LDS_BYTES + OpB::LDS_BYTES;
    constexpr int KB = BK / Frag::KPB;      // k-blocks per K-tile
    static_assert(BK % Frag::KPB == 0 && KB >= 1, "whole k-blocks");
    static_assert(2 * STAGE <= 65536, "static LDS");
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

    const double* A = static_cast<const double*>(p.A) + group_offset<0>(p.gL, l) * (int64_t)SD;
    const double* B = static_cast<const double*>(p.B) + group_offset<1>(p.gL, l) * (int64_t)SD;

    OpA ta;
    OpB tb;
    ta.template init_rows<0>(p.gM, m0, tid);
    tb.template init_rows<0>(p.gN, n0, tid);
    const bool conjA = CPLX && p.conjA != 0, conjB = CPLX && p.conjB != 0;

    F64xAcc<CPLX> acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if constexpr (CPLX) {
                acc[i][j].rr = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][j].ii = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][j].x = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                acc[i][j].v = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }

    // per-lane byte offsets of the fragment units (the swizzle has a period of 16 rows: valid for every 16-row block)
    int fragOff[KB][Frag::UPL];
#pragma unroll
    for (int s = 0; s < KB; ++s)
#pragma unroll
        for (int h = 0; h < Frag::UPL; ++h) fragOff[s][h] = Img::unit_addr(0, r, Frag::unit(s, q, h));

    auto compute = [&](const char* buf) {
        const char* la = buf + (wm * (BM / WM)) * Img::RB;
        const char* lb = buf + OpA::LDS_BYTES + (wn * (BN / Cfg::WN)) * Img::RB;
#pragma unroll
        for (int s = 0; s < KB; ++s) {
            if constexpr (!CPLX) {
                f32x4 fa[TM], fb[TN];       // elements k = 4 (4 s + q) + j of the row
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(la + 16 * i * Img::RB + fragOff[s][0]);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(lb + 16 * j * Img::RB + fragOff[s][0]);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j].v = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][kk], fb[j][kk], acc[i][j].v, 0, 0, 0);
            } else {
                f32x4 fa[TM][2], fb[TN][2];   // [h]: elements 2 h, 2 h + 1 as (re, im, re, im)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h) fa[i][h] = *reinterpret_cast<const f32x4*>(la + 16 * i * Img::RB + fragOff[s][h]);
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int h = 0; h < 2; ++h) fb[j][h] = *reinterpret_cast<const f32x4*>(lb + 16 * j * Img::RB + fragOff[s][h]);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            const float are = fa[i][kk >> 1][2 * (kk & 1)], aim = fa[i][kk >> 1][2 * (kk & 1) + 1];
                            const float bre = fb[j][kk >> 1][2 * (kk & 1)], bim = fb[j][kk >> 1][2 * (kk & 1) + 1];
                            acc[i][j].rr = __builtin_amdgcn_mfma_f32_16x16x4f32(are, bre, acc[i][j].rr, 0, 0, 0);
                            acc[i][j].ii = __builtin_amdgcn_mfma_f32_16x16x4f32(aim, bim, acc[i][j].ii, 0, 0, 0);
                            acc[i][j].x  = __builtin_amdgcn_mfma_f32_16x16x4f32(are, bim, acc[i][j].x, 0, 0, 0);
                            acc[i][j].x  = __builtin_amdgcn_mfma_f32_16x16x4f32(aim, bre, acc[i][j].x, 0, 0, 0);
                        }
            }
        }
    };

    // ---- main loop: loads of tile t + 1 in flight under the MFMAs of tile t -------------------------------------------------
    const int nTiles = (kEnd > kBegin) ? (int)((kEnd - kBegin + BK - 1) / BK) : 0;
    double sa[OpA::NU][OpA::ND], sb[OpB::NU][OpB::ND];
    bool oka = false, okb = false;
    if (nTiles > 0) {
        oka = ta.template load<0, 0>(sa, A, p.gM, p.gK, kBegin, kEnd, tid);
        okb = tb.template load<0, 1>(sb, B, p.gN, p.gK, kBegin, kEnd, tid);
        ta.store(sa, oka, conjA, lds, tid);
        tb.store(sb, okb, conjB, lds + OpA::LDS_BYTES, tid);
    }
    __syncthreads();
    for (int t = 0; t < nTiles; ++t) {
        const bool more = t + 1 < nTiles;
        if (more) {
            oka = ta.template load<0, 0>(sa, A, p.gM, p.gK, kBegin + (uint32_t)(t + 1) * BK, kEnd, tid);
            okb = tb.template load<0, 1>(sb, B, p.gN, p.gK, kBegin + (uint32_t)(t + 1) * BK, kEnd, tid);
        }
        compute(lds + (t & 1) * STAGE);
        if (more) {
            char* nxt = lds + ((t + 1) & 1) * STAGE;      // last read by the MFMAs of tile t - 1: every wave is past that barrier
            ta.store(sa, oka, conjA, nxt, tid);
            tb.store(sb, okb, conjB, nxt + OpA::LDS_BYTES, tid);
        }
        __syncthreads();
    }

    // ---- epilogue (fp64) --------------------------------------------------------------------------------------------------
    // accumulator register t of a fragment: row 4 q + t, column r
    const uint32_t Mtot = p.gM.total, Ntot = p.gN.total;
    const uint32_t mBase = m0 + wm * (BM / WM), nBase = n0 + wn * (BN / Cfg::WN);
    if (p.partial != nullptr) {
        // split-K: fp32 / float2 partial tiles [slice][L][M][N], folded in fp64 by launch_gen_splitk_reduce
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
                    const size_t e = tileOff + (size_t)m * Ntot + n;
                    if constexpr (CPLX) reinterpret_cast<f32x2*>(p.partial)[e] = f32x2{acc[i][j].rr[t] - acc[i][j].ii[t], acc[i][j].x[t]};
                    else                p.partial[e] = acc[i][j].v[t];
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
                if constexpr (!CPLX) {
                    double val = p.alpha64 * (double)acc[i][j].v[t];
                    if (p.beta64 != 0.0) val += p.beta64 * static_cast<const double*>(p.C)[oC];
                    static_cast<double*>(p.D)[oD] = val;
                } else {
                    const double re = (double)acc[i][j].rr[t] - (double)acc[i][j].ii[t], im = (double)acc[i][j].x[t];
                    const double alRe = p.alpha64, alIm = p.alphaIm, beRe = p.beta64, beIm = p.betaIm;
                    // (a real alpha scales: 0 * inf of the general product would turn an infinite result into NaN)
                    double oRe = alRe * re, oIm = alRe * im;
                    if (alIm != 0.0) { oRe -= alIm * im; oIm += alIm * re; }
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
}

#define CTAMD_F64X_ORIENTS(GE, BM, BN, BK, V) CTAMD_GEN_FAMILY_ORIENTS(gett_gen_f64x_kernel, F64xCfg, GE, BM, BN, BK, V)

}  // namespace ctamd
