// gett_gen.inc — the GENERAL MFMA GETT kernel for gfx950: any strides, any extents, five element types.
//
// The aligned kernels (gett_h16*.hip: LDS-DMA, 16-byte lanes, whole 64-deep K-tiles; gett_f32*.hip) cover the shapes the
// benchmarks are quoted on.  Everything else used to fall to the one-output-per-lane FMA kernels of gett_simple.hip — among it
// every 16-bit case of the reference's own regression list (cuTENSOR/python/cutensor/torch/einsum_test.py:84-123: extents of
// 50, no 16-byte lanes, K not a multiple of 64), all fp64 contractions (cuTENSOR/einsum.cu:36-41 with double,
// einsum_test.py:109-115) and all complex ones (python/einsum.h:51-63, einsum_test.py:55-68, contraction_jit.cu:39-42).
// This kernel puts them on the matrix cores:
//
//   element type        MFMA                               accumulators per 16 x 16 fragment
//   bf16 / fp16         v_mfma_f32_16x16x32_{bf16,f16}     1 x fp32x4
//   fp64                v_mfma_f64_16x16x4_f64             1 x fp64x4
//   complex64           v_mfma_f32_16x16x4_f32 x 4         3 x fp32x4  (Re·Re, Im·Im, Re·Im + Im·Re)
//   complex128          v_mfma_f64_16x16x4_f64 x 4         3 x fp64x4
//
// Structure (one source for all of them): a workgroup of 256 threads (2 x 2 waves) owns a BM x BN output tile.  Every
// thread stages NU "units" of each operand per K-tile: V consecutive elements along the operand's contiguous direction (k for
// a K-contiguous operand, rows for a free-contiguous one), ONE global load of V * ES bytes each — V = 8 / 2 / 1 for 16-bit
// data (16-byte lanes, 4-byte pairs, 2-byte gathers), 2 / 1 for fp64 and complex64, 1 for complex128; the planner picks the
// largest V both operands' strides, extents and alignment admit.  Rows beyond the tensor edge are clamped to a valid row (they
// feed accumulators that are never stored); k beyond the K range loads a clamped address and is ZEROED on its way into LDS, so
// K needs no padding and no divisibility.  The units go through registers into a [row][k] LDS image (gett_gen_layout.h: 16-byte
// units XOR-swizzled, conflict-free b128 fragment reads; a free-contiguous operand is transposed by the staging writes), two
// LDS buffers, the global loads of tile t + 1 in flight under the MFMAs of tile t, one barrier per K-tile.  The contracted index
// is decoded once per thread and K-tile (all units of a thread share their k): a multiplication when the contracted modes fused
// into one, the mixed-radix decode otherwise.  Conjugation of a complex input is a sign flip on the staged imaginary parts.
// Epilogue: D = alpha * acc + beta * op(C) straight from the accumulators (lanes along n, the mode D is contiguous in), or fp32
// partial tiles [slice][L][M][N] for split-K of 16-bit data (folded by launch_splitk_reduce with one rounding).
//
// Split-K (few output tiles, long K): every slice writes its tile in the accumulator type, a second small kernel folds.
//
// Included by gett_gen_h16.hip / gett_gen_f64.hip / gett_gen_cplx.hip, which instantiate their part of the table.
#include "gett_gen_common.h"
#include "round16.h"

namespace ctamd {

template <int GE> struct GenElemTraits;
template <> struct GenElemTraits<GEN_BF16> { static constexpr int ES = 2;  static constexpr bool ACC64 = false, CPLX = false; };
template <> struct GenElemTraits<GEN_F16>  { static constexpr int ES = 2;  static constexpr bool ACC64 = false, CPLX = false; };
template <> struct GenElemTraits<GEN_F64>  { static constexpr int ES = 8;  static constexpr bool ACC64 = true,  CPLX = false; };
template <> struct GenElemTraits<GEN_C32>  { static constexpr int ES = 8;  static constexpr bool ACC64 = false, CPLX = true;  };
template <> struct GenElemTraits<GEN_C64>  { static constexpr int ES = 16; static constexpr bool ACC64 = true,  CPLX = true;  };

template <int GE_, int BM_, int BN_, int BK_, int OA_, int OB_, int V_>
struct GenCfg {
    static constexpr int GE = GE_, BM = BM_, BN = BN_, BK = BK_, OA = OA_, OB = OB_, V = V_;
    static constexpr int WM = 2, WN = 2, THREADS = 256;
    static constexpr int TM = BM / (WM * 16), TN = BN / (WN * 16);
    using T = GenElemTraits<GE>;
    static_assert(BM % 32 == 0 && BN % 32 == 0, "wave sub-tiles are 16-granular");
};

// ---------------------------------------------------------------------------------------------
// One operand of the K-tile: global -> registers -> LDS.
// ---------------------------------------------------------------------------------------------
// (ImgT: the LDS image — GenImage of the element size and K-tile, but for gett_gen_rc64.inc's real operand)
template <int ES, int ORIENT, int ROWS, int BK, int V, class ImgT = GenImage<ES, BK>>
struct GenOperand {
    using Map = GenUnitMap<ORIENT, ROWS, BK, V, 256>;
    using Img = ImgT;
    static constexpr int NU = Map::NU;
    static constexpr int UB = V * ES;                  // bytes per unit = per global load: 2, 4, 8 or 16
    static constexpr int DW = UB >= 4 ? UB / 4 : 1;    // staging dwords per unit
    static_assert(UB == 2 || UB == 4 || UB == 8 || UB == 16, "one load instruction per unit");
    static constexpr int LDS_BYTES = ROWS * Img::RB;

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
    __device__ __forceinline__ bool load(uint32_t (&st)[NU][DW], const char* __restrict__ X, const ModeGroup& gK, uint32_t k0, uint32_t kEnd,
                                         int tid) const {
        const uint32_t k = k0 + (uint32_t)Map::unit_k(tid);
        const bool ok = k < kEnd;
        const uint32_t kc = ok ? k : kEnd - (ORIENT ? (uint32_t)V : 1u);      // K-contiguous units: the K range is a multiple of V
        const int64_t offK = (gK.n <= 1) ? (int64_t)kc * gK.stride[SLOT_K][0] : group_offset<SLOT_K>(gK, kc);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const char* src = X + (rowOff[i] + offK) * (int64_t)ES;
            if constexpr (UB == 16) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(src);
                st[i][0] = v[0]; st[i][1] = v[1]; st[i][2] = v[2]; st[i][3] = v[3];
            } else if constexpr (UB == 8) {
                const u32x2 v = *reinterpret_cast<const u32x2*>(src);
                st[i][0] = v[0]; st[i][1] = v[1];
            } else if constexpr (UB == 4) {
                st[i][0] = *reinterpret_cast<const uint32_t*>(src);
            } else {
                st[i][0] = *reinterpret_cast<const uint16_t*>(src);
            }
        }
        return ok;
    }

    // Registers -> LDS image.  conj (complex data): flip the sign of the imaginary parts on the way.
    template <bool CPLX>
    __device__ __forceinline__ void store(const uint32_t (&st)[NU][DW], bool ok, bool conj, char* lds, int tid) const {
        const int kl = Map::unit_k(tid);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            uint32_t w[DW];
#pragma unroll
            for (int d = 0; d < DW; ++d) w[d] = ok ? st[i][d] : 0u;
            if constexpr (CPLX) {
                // complex64: dwords (re, im) per element; complex128: (re lo, re hi, im lo, im hi)
                if (conj) {
                    if constexpr (ES == 8) {
#pragma unroll
                        for (int d = 1; d < DW; d += 2) w[d] ^= 0x80000000u;
                    } else {
                        w[3] ^= 0x80000000u;
                    }
                }
            }
            const int row = Map::unit_row(tid, i);
            if constexpr (ORIENT == 1 || V == 1) {
                char* dst = lds + Img::addr(row, kl);
                if constexpr (UB == 16)     *reinterpret_cast<u32x4*>(dst) = u32x4{w[0], w[1], w[2], w[3]};
                else if constexpr (UB == 8) *reinterpret_cast<u32x2*>(dst) = u32x2{w[0], w[1]};
                else if constexpr (UB == 4) *reinterpret_cast<uint32_t*>(dst) = w[0];
                else                        *reinterpret_cast<uint16_t*>(dst) = (uint16_t)w[0];
            } else {
                // free-contiguous unit: V rows at one k — the transposition happens here
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    char* dst = lds + Img::addr(row + e, kl);
                    if constexpr (ES == 2)      *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
                    else if constexpr (ES == 8) *reinterpret_cast<u32x2*>(dst) = u32x2{w[2 * e], w[2 * e + 1]};
                }
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------
// MFMA step of one k-block for the TM x TN fragments of a wave.
// ---------------------------------------------------------------------------------------------
template <int GE> struct GenAcc;
template <> struct GenAcc<GEN_BF16> { f32x4 v; };
template <> struct GenAcc<GEN_F16>  { f32x4 v; };
template <> struct GenAcc<GEN_F64>  { f64x4 v; };
template <> struct GenAcc<GEN_C32>  { f32x4 rr, ii, x; };
template <> struct GenAcc<GEN_C64>  { f64x4 rr, ii, x; };

template <class Cfg>
__global__ void __launch_bounds__(256, 2) gett_gen_kernel(const GettParams p) {
    constexpr int GE = Cfg::GE, BM = Cfg::BM, BN = Cfg::BN, BK = Cfg::BK, V = Cfg::V;
    constexpr int WM = Cfg::WM, TM = Cfg::TM, TN = Cfg::TN;
    using T = typename Cfg::T;
    constexpr int ES = T::ES;
    using OpA = GenOperand<ES, Cfg::OA, BM, BK, V>;
    using OpB = GenOperand<ES, Cfg::OB, BN, BK, V>;
    using Img = GenImage<ES, BK>;
    using Frag = GenFrag<ES>;
    constexpr int STAGE = OpA::LDS_BYTES + OpB::LDS_BYTES;
    constexpr int KB = BK / Frag::KPB;      // k-blocks per K-tile
    static_assert(BK % Frag::KPB == 0 && KB >= 1, "whole k-blocks");
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

    const char* A = static_cast<const char*>(p.A) + group_offset<0>(p.gL, l) * (int64_t)ES;
    const char* B = static_cast<const char*>(p.B) + group_offset<1>(p.gL, l) * (int64_t)ES;

    OpA ta;
    OpB tb;
    ta.template init_rows<0>(p.gM, m0, tid);
    tb.template init_rows<0>(p.gN, n0, tid);
    const bool conjA = T::CPLX && p.conjA != 0, conjB = T::CPLX && p.conjB != 0;

    GenAcc<GE> acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if constexpr (!T::CPLX) {
                if constexpr (T::ACC64) acc[i][j].v = f64x4{0., 0., 0., 0.};
                else                    acc[i][j].v = f32x4{0.f, 0.f, 0.f, 0.f};
            } else if constexpr (T::ACC64) {
                acc[i][j].rr = f64x4{0., 0., 0., 0.}; acc[i][j].ii = f64x4{0., 0., 0., 0.}; acc[i][j].x = f64x4{0., 0., 0., 0.};
            } else {
                acc[i][j].rr = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][j].ii = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][j].x = f32x4{0.f, 0.f, 0.f, 0.f};
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
            if constexpr (ES == 2) {
                g16x8 fa[TM], fb[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const g16x8*>(la + 16 * i * Img::RB + fragOff[s][0]);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const g16x8*>(lb + 16 * j * Img::RB + fragOff[s][0]);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        acc[i][j].v = gen_mfma16<GE == GEN_F16>(fa[i], fb[j], acc[i][j].v);
                    }
            } else if constexpr (GE == GEN_F64) {
                f64x4 fa[TM], fb[TN];       // elements k = 4 q + j of the row
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const f64x2 a0 = *reinterpret_cast<const f64x2*>(la + 16 * i * Img::RB + fragOff[s][0]);
                    const f64x2 a1 = *reinterpret_cast<const f64x2*>(la + 16 * i * Img::RB + fragOff[s][1]);
                    fa[i] = f64x4{a0[0], a0[1], a1[0], a1[1]};
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const f64x2 b0 = *reinterpret_cast<const f64x2*>(lb + 16 * j * Img::RB + fragOff[s][0]);
                    const f64x2 b1 = *reinterpret_cast<const f64x2*>(lb + 16 * j * Img::RB + fragOff[s][1]);
                    fb[j] = f64x4{b0[0], b0[1], b1[0], b1[1]};
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j].v = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i][kk], fb[j][kk], acc[i][j].v, 0, 0, 0);
            } else if constexpr (GE == GEN_C32) {
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
            } else {   // GEN_C64: elements k = 2 q + h as (re, im)
                f64x4 fa[TM], fb[TN];         // (re0, im0, re1, im1)
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const f64x2 a0 = *reinterpret_cast<const f64x2*>(la + 16 * i * Img::RB + fragOff[s][0]);
                    const f64x2 a1 = *reinterpret_cast<const f64x2*>(la + 16 * i * Img::RB + fragOff[s][1]);
                    fa[i] = f64x4{a0[0], a0[1], a1[0], a1[1]};
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const f64x2 b0 = *reinterpret_cast<const f64x2*>(lb + 16 * j * Img::RB + fragOff[s][0]);
                    const f64x2 b1 = *reinterpret_cast<const f64x2*>(lb + 16 * j * Img::RB + fragOff[s][1]);
                    fb[j] = f64x4{b0[0], b0[1], b1[0], b1[1]};
                }
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            const double are = fa[i][2 * kk], aim = fa[i][2 * kk + 1];
                            const double bre = fb[j][2 * kk], bim = fb[j][2 * kk + 1];
                            acc[i][j].rr = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bre, acc[i][j].rr, 0, 0, 0);
                            acc[i][j].ii = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, bim, acc[i][j].ii, 0, 0, 0);
                            acc[i][j].x  = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bim, acc[i][j].x, 0, 0, 0);
                            acc[i][j].x  = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, bre, acc[i][j].x, 0, 0, 0);
                        }
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
        ta.template store<T::CPLX>(sa, oka, conjA, lds, tid);
        tb.template store<T::CPLX>(sb, okb, conjB, lds + OpA::LDS_BYTES, tid);
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
            ta.template store<T::CPLX>(sa, oka, conjA, nxt, tid);
            tb.template store<T::CPLX>(sb, okb, conjB, nxt + OpA::LDS_BYTES, tid);
        }
        __syncthreads();
    }

    // ---- epilogue ---------------------------------------------------------------------------------------------------------
    // accumulator register t of a fragment: row gen_acc_row(q, t), column r
    const uint32_t Mtot = p.gM.total, Ntot = p.gN.total;
    const uint32_t mBase = m0 + wm * (BM / WM), nBase = n0 + wn * (BN / Cfg::WN);
    if (p.partial != nullptr) {
        // split-K: partial tiles [slice][L][M][N] in the accumulator type — fp32 for 16-bit data (folded by launch_splitk_reduce with
        // one rounding), double / float2 / double2 for fp64 / complex64 / complex128 (launch_gen_splitk_reduce)
        const size_t tileOff = ((size_t)slice * p.gL.total + l) * (size_t)Mtot * Ntot;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t m = mBase + 16 * i + gen_acc_row<T::ACC64>(q, t);
                if (m >= Mtot) continue;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const uint32_t n = nBase + 16 * j + r;
                    if (n >= Ntot) continue;
                    const size_t e = tileOff + (size_t)m * Ntot + n;
                    if constexpr (ES == 2) p.partial[e] = acc[i][j].v[t];
                    else if constexpr (GE == GEN_F64) reinterpret_cast<double*>(p.partial)[e] = acc[i][j].v[t];
                    else if constexpr (GE == GEN_C32) {
                        reinterpret_cast<f32x2*>(p.partial)[e] = f32x2{acc[i][j].rr[t] - acc[i][j].ii[t], acc[i][j].x[t]};
                    } else
                        reinterpret_cast<f64x2*>(p.partial)[e] = f64x2{acc[i][j].rr[t] - acc[i][j].ii[t], acc[i][j].x[t]};
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
            const uint32_t m = mBase + 16 * i + gen_acc_row<T::ACC64>(q, t);
            if (m >= Mtot) continue;
            int64_t offDm, offCm;
            if (flat) { offDm = (int64_t)m * p.gM.stride[1][0]; offCm = (int64_t)m * p.cStrideM[0]; }
            else group_offset2<1>(p.gM, p.cStrideM, m, offDm, offCm);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (!okN[j]) continue;
                const int64_t oD = offDm + offDn[j], oC = offCm + offCn[j];
                if constexpr (ES == 2) {
                    constexpr bool BF = GE == GEN_BF16;
                    const float val = p.alpha * acc[i][j].v[t];      // one rounding of val + beta * c: round16.h
                    static_cast<uint16_t*>(p.D)[oD] = p.beta != 0.f ? h_round16_with_c<BF>(val, p.beta, static_cast<const uint16_t*>(p.C)[oC])
                                                                      : h_round16<BF>(val);
                } else if constexpr (GE == GEN_F64) {
                    double val = p.alpha64 * acc[i][j].v[t];
                    if (p.beta64 != 0.0) val += p.beta64 * static_cast<const double*>(p.C)[oC];
                    static_cast<double*>(p.D)[oD] = val;
                } else if constexpr (GE == GEN_C32) {
                    const float re = acc[i][j].rr[t] - acc[i][j].ii[t], im = acc[i][j].x[t];
                    const float alRe = (float)p.alpha64, alIm = (float)p.alphaIm, beRe = (float)p.beta64, beIm = (float)p.betaIm;
                    float oRe = alRe * re - alIm * im, oIm = alRe * im + alIm * re;
                    if (beRe != 0.f || beIm != 0.f) {
                        const float* c = static_cast<const float*>(p.C) + 2 * oC;
                        const float cRe = c[0], cIm = p.conjC ? -c[1] : c[1];
                        oRe += beRe * cRe - beIm * cIm;
                        oIm += beRe * cIm + beIm * cRe;
                    }
                    *reinterpret_cast<f32x2*>(static_cast<float*>(p.D) + 2 * oD) = f32x2{oRe, oIm};
                } else {
                    const double re = acc[i][j].rr[t] - acc[i][j].ii[t], im = acc[i][j].x[t];
                    const double alRe = p.alpha64, alIm = p.alphaIm, beRe = p.beta64, beIm = p.betaIm;
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
}

#define CTAMD_GEN_ORIENTS(GE, BM, BN, BK, V) CTAMD_GEN_FAMILY_ORIENTS(gett_gen_kernel, GenCfg, GE, BM, BN, BK, V)

}  // namespace ctamd
