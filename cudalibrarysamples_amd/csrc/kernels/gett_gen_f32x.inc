// gett_gen_f32x.inc — fp32 DATA on the 16-bit matrix rate: the reduced-precision compute descriptors of a real fp32 contraction.
//
//   compute descriptor   products                                            MFMA per k-block and fragment pair
//   COMPUTE_DESC_16BF    bf16(a) * bf16(b)                                   v_mfma_f32_16x16x32_bf16 x 1
//   COMPUTE_DESC_16F     fp16(a) * fp16(b)  (|x| > 65504 becomes +-inf)      v_mfma_f32_16x16x32_f16  x 1
//   COMPUTE_DESC_TF32    hi_a hi_b + hi_a lo_b + lo_a hi_b                   v_mfma_f32_16x16x32_bf16 x 3, one accumulator
//                        hi = bf16(x), lo = bf16(x - hi)  (x - hi is exact in fp32; the split drops lo_a lo_b and the two second
//                        roundings: 3 u^2 per product with u = 2^-8)
//
// gfx950 has no TF32 / xf32 MFMA, so the request is served by rounding (and, for TF32, splitting) the fp32 operands on their way
// into LDS.  The structure is that of gett_gen.inc — 256 threads, 2 x 2 waves, every thread stages NU units of V fp32 elements
// per operand and K-tile (V = 4: one 16-byte load, V = 1: 4-byte gathers; LAY_F / LAY_K per operand), two LDS stages, the loads
// of tile t + 1 in flight under the MFMAs of tile t, one barrier per K-tile, rows clamped at the M / N edges, k past the K end
// zeroed, mixed-radix decode of a multi-digit K, xcd_remap, fp32 split-K partials [slice][L][M][N] for launch_splitk_reduce —
// with the conversion between the global load and the LDS write.  The LDS side is the 16-bit image of gett_gen_layout.h
// (GenImage<2, BK>, GenFrag<2>: the searched, conflict-free swizzles): one image per operand for 16BF / 16F, two (hi, lo) for TF32.
// Epilogue in fp32: D = alpha * acc + beta * C, any strides, C never read when beta == 0.
//
// Non-finite values under TF32: x whose bf16 rounding is not finite (inf, NaN, |x| >= 2^128 (1 - 2^-9)) goes to the LO plane as it is,
// with hi = 0.  Then inf * b arrives as lo_a * hi_b = inf * bf16(b) with the right sign, and the other two terms are 0 * finite = 0.
// (With the non-finite value in the hi plane, hi_a * lo_b would be inf * 0 = NaN or inf of the wrong sign for every b that is not
// a bf16 value.)  Two non-finite factors meeting in one product give NaN.
//
// LDS budget (static, two stages): 128 x 128 x 64 one image: 64 KiB; 128 x 128 x 32 two images: 64 KiB; two workgroups per CU.
#include "gett_gen_common.h"

namespace ctamd {

template <int GE_, int BM_, int BN_, int BK_, int OA_, int OB_, int V_>
struct F32xCfg {
    static constexpr int GE = GE_, BM = BM_, BN = BN_, BK = BK_, OA = OA_, OB = OB_, V = V_;
    static constexpr int WM = 2, WN = 2, THREADS = 256;
    static constexpr int TM = BM / (WM * 16), TN = BN / (WN * 16);
    using Cvt = Gen16Cvt<GE - GEN_F32_BF16>;
    static constexpr int PLANES = Cvt::PLANES;
    static_assert(BM % 32 == 0 && BN % 32 == 0, "wave sub-tiles are 16-granular");
    static_assert(V == 4 || V == 1, "16-byte loads or 4-byte gathers");
};

// ---------------------------------------------------------------------------------------------
// One operand of the K-tile: global fp32 -> registers -> (rounded) 16-bit LDS image(s).
// ---------------------------------------------------------------------------------------------
template <class Cvt, int ORIENT, int ROWS, int BK, int V>
struct F32xOperand {
    using Map = GenUnitMap<ORIENT, ROWS, BK, V, 256>;
    using Img = GenImage<2, BK>;
    static constexpr int NU = Map::NU;
    static constexpr int PLANE_BYTES = ROWS * Img::RB;
    static constexpr int LDS_BYTES = Cvt::PLANES * PLANE_BYTES;

    int64_t rowOff[NU];      // element offset of each unit's first row in the operand (clamped to a valid row)

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

    // Issue the loads of the K-tile at k0.  Returns whether this thread's k lies inside [k0, kEnd) (if not, a clamped valid
    // address was loaded and store() writes zeros).
    template <int SLOT_K>
    __device__ __forceinline__ bool load(float (&st)[NU][V], const float* __restrict__ X, const ModeGroup& gK, uint32_t k0, uint32_t kEnd,
                                         int tid) const {
        const uint32_t k = k0 + (uint32_t)Map::unit_k(tid);
        const bool ok = k < kEnd;
        const uint32_t kc = ok ? k : kEnd - (ORIENT ? (uint32_t)V : 1u);      // K-contiguous units: the K range is a multiple of V
        const int64_t offK = (gK.n <= 1) ? (int64_t)kc * gK.stride[SLOT_K][0] : group_offset<SLOT_K>(gK, kc);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const float* src = X + (rowOff[i] + offK);
            if constexpr (V == 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src);
                st[i][0] = v[0]; st[i][1] = v[1]; st[i][2] = v[2]; st[i][3] = v[3];
            } else {
                st[i][0] = *src;
            }
        }
        return ok;
    }

    // Registers -> LDS: round (split) each element, write plane pl at lds + pl * PLANE_BYTES
    __device__ __forceinline__ void store(const float (&st)[NU][V], bool ok, char* lds, int tid) const {
        const int kl = Map::unit_k(tid);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            uint16_t h[V][Cvt::PLANES];
#pragma unroll
            for (int e = 0; e < V; ++e) Cvt::cvt(ok ? st[i][e] : 0.f, h[e]);
            const int row = Map::unit_row(tid, i);
#pragma unroll
            for (int pl = 0; pl < Cvt::PLANES; ++pl) {
                char* base = lds + pl * PLANE_BYTES;
                if constexpr (V == 1) {
                    *reinterpret_cast<uint16_t*>(base + Img::addr(row, kl)) = h[0][pl];
                } else if constexpr (ORIENT == 1) {
                    // four consecutive k of one row: 8 bytes inside one 16-byte unit of the image
                    *reinterpret_cast<u32x2*>(base + Img::addr(row, kl)) =
                        u32x2{(uint32_t)h[0][pl] | ((uint32_t)h[1][pl] << 16), (uint32_t)h[2][pl] | ((uint32_t)h[3][pl] << 16)};
                } else {
                    // free-contiguous unit: V rows at one k — the transposition happens here
#pragma unroll
                    for (int e = 0; e < V; ++e) *reinterpret_cast<uint16_t*>(base + Img::addr(row + e, kl)) = h[e][pl];
                }
            }
        }
    }
};

template <class Cfg>
__global__ void __launch_bounds__(256, 2) gett_gen_f32x_kernel(const GettParams p) {
    constexpr int GE = Cfg::GE, BM = Cfg::BM, BN = Cfg::BN, BK = Cfg::BK, V = Cfg::V;
    constexpr int WM = Cfg::WM, TM = Cfg::TM, TN = Cfg::TN, PLANES = Cfg::PLANES;
    using OpA = F32xOperand<typename Cfg::Cvt, Cfg::OA, BM, BK, V>;
    using OpB = F32xOperand<typename Cfg::Cvt, Cfg::OB, BN, BK, V>;
    using Img = GenImage<2, BK>;
    using Frag = GenFrag<2>;
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

    const float* A = static_cast<const float*>(p.A) + group_offset<0>(p.gL, l);
    const float* B = static_cast<const float*>(p.B) + group_offset<1>(p.gL, l);

    OpA ta;
    OpB tb;
    ta.template init_rows<0>(p.gM, m0, tid);
    tb.template init_rows<0>(p.gN, n0, tid);

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-lane byte offset of the fragment unit (the swizzle has a period of 16 rows: valid for every 16-row block)
    int fragOff[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) fragOff[s] = Img::unit_addr(0, r, Frag::unit(s, q, 0));

    constexpr bool F16 = GE == GEN_F32_F16;
    auto compute = [&](const char* buf) {
        const char* la = buf + (wm * (BM / WM)) * Img::RB;
        const char* lb = buf + OpA::LDS_BYTES + (wn * (BN / Cfg::WN)) * Img::RB;
#pragma unroll
        for (int s = 0; s < KB; ++s) {
            g16x8 fa[PLANES][TM], fb[PLANES][TN];
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[pl][i] = *reinterpret_cast<const g16x8*>(la + pl * OpA::PLANE_BYTES + 16 * i * Img::RB + fragOff[s]);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[pl][j] = *reinterpret_cast<const g16x8*>(lb + pl * OpB::PLANE_BYTES + 16 * j * Img::RB + fragOff[s]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (PLANES == 2) {      // the two small terms first, then hi * hi: all into the same accumulator
                        acc[i][j] = gen_mfma16<F16>(fa[1][i], fb[0][j], acc[i][j]);
                        acc[i][j] = gen_mfma16<F16>(fa[0][i], fb[1][j], acc[i][j]);
                    }
                    acc[i][j] = gen_mfma16<F16>(fa[0][i], fb[0][j], acc[i][j]);
                }
        }
    };

    // ---- main loop: loads of tile t + 1 in flight under the MFMAs of tile t -------------------------------------------------
    const int nTiles = (kEnd > kBegin) ? (int)((kEnd - kBegin + BK - 1) / BK) : 0;
    float sa[OpA::NU][V], sb[OpB::NU][V];
    bool oka = false, okb = false;
    if (nTiles > 0) {
        oka = ta.template load<0>(sa, A, p.gK, kBegin, kEnd, tid);
        okb = tb.template load<1>(sb, B, p.gK, kBegin, kEnd, tid);
        ta.store(sa, oka, lds, tid);
        tb.store(sb, okb, lds + OpA::LDS_BYTES, tid);
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
            ta.store(sa, oka, nxt, tid);
            tb.store(sb, okb, nxt + OpA::LDS_BYTES, tid);
        }
        __syncthreads();
    }

    // ---- epilogue (fp32) --------------------------------------------------------------------------------------------------
    // accumulator register t of a fragment: row 4 q + t, column r
    const uint32_t Mtot = p.gM.total, Ntot = p.gN.total;
    const uint32_t mBase = m0 + wm * (BM / WM), nBase = n0 + wn * (BN / Cfg::WN);
    if (p.partial != nullptr) {
        // split-K: fp32 partial tiles [slice][L][M][N], folded by launch_splitk_reduce (output type fp32)
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
                    p.partial[tileOff + (size_t)m * Ntot + n] = acc[i][j][t];
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
                float val = p.alpha * acc[i][j][t];
                if (p.beta != 0.f) val += p.beta * static_cast<const float*>(p.C)[offCm + offCn[j]];
                static_cast<float*>(p.D)[offDm + offDn[j]] = val;
            }
        }
}

#define CTAMD_F32X_ORIENTS(GE, BM, BN, BK, V) CTAMD_GEN_FAMILY_ORIENTS(gett_gen_f32x_kernel, F32xCfg, GE, BM, BN, BK, V)

}  // namespace ctamd
