// elementwise_convert.hip — the converting twins of the element-wise kernels for gfx950: cutensorPermute and
// cutensorElementwiseBinaryExecute with an output (and C) whose data type differs from A's.
//
//   D = rnd_D( opAC( alpha * unA(cmp(perm A)), gamma * unC(cmp(C)) ) )          C has D's type
//
// Pairs (A -> D): bf16 / fp16 -> fp32 and fp32 -> bf16 / fp16 (cmp = fp32), fp32 -> fp64 and fp64 -> fp32 (cmp = fp64).  The loaded
// element is widened to cmp (exact), the unary operator, the scalar and the combiner act in cmp, and ONE rounding to nearest even into
// D's type ends it: overflow gives +-inf, D's subnormals are produced, NaN stays (quiet) NaN, -0 stays -0.  HBM-bound; algorithmic
// bytes per element = sizeof A + sizeof D (+ sizeof D when the gamma * C term is read).
//
// The unit is a lane of LV = 16 / min(sizeof A, sizeof D) elements (8 for the 16 <-> 32 pairs, 4 for 32 <-> 64): one 16-byte access
// on the narrow side, two on the wide side.  Same tile decomposition (Ew2DParams), tile orders and variant numbers as elementwise.hip:
//
//   EW_ROWCOPY    A and D share the stride-1 mode: lanes along dim0, 64 x LV elements x 8 dim1 rows per workgroup, no LDS,
//                 nontemporal loads and stores.
//   EW_TRANSPOSE  D contiguous along dim0, A along dim1.  A T0 x 64 tile is read in LV x LV blocks (LV rows of dim0, LV elements
//                 along dim1 per lane), transposed in registers and parked in LDS as [dim1][dim0] in the NARROWER type: when
//                 narrowing, alpha * unA(a) is rounded to D's type before parking and the write phase is a copy; when widening, A's
//                 bits are parked and the arithmetic follows the LDS read.  The one exception keeps the single rounding: a narrowing
//                 plan WITH a C term parks A's bits (the combiner needs alpha * unA(a) unrounded), on tiles half as wide.
//                 LDS rows are T0 elements with the 16-byte piece index XOR-swizzled by the row's block ((row / LV) & 7): the eight
//                 lanes of a ds_write_b128 group (eight dim1 blocks, one dim0 block) land on eight different 16-byte slots, and the
//                 rows read back by a ds_read_b128 group are whole rows, a permutation of their slots.  T0 (planner): the widest of
//                 256 / 128 / 64 the extent fills and 32 KiB of LDS hold: written row segments of 512 B and more, read segments of
//                 128 B (16-bit A) / 256 B (fp32 A) / 512 B (fp64 A).  One workgroup per tile, interior tiles unguarded with every
//                 load issued before the first use, edge tiles guarded per LV group.
//   EW_GENERIC    anything else (odd extents, strides of 0, unaligned bases, padded permutations): one element per lane.
//
// EW_TRANSPOSE_ANY and EW_BLOCK have no converting twin: such problems take the generic form.
// Every kernel exists with and without the C term and with and without the unary operators (template flags HASC / UN; the identity
// instantiations compile none of unary_op.h's switch).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "elementwise_common.h"
#include "launch.h"
#include "params.h"
#include "unary_op.h"

namespace ctamd {

// element kinds: storage type, widening to the compute type S (exact), rounding from it (to nearest even)
struct CvF32 {
    typedef float Elem;
    template <typename S> static __device__ __forceinline__ S to(float v) { return (S)v; }
    template <typename S> static __device__ __forceinline__ float from(S v) { return (float)v; }
};
struct CvF64 {
    typedef double Elem;
    template <typename S> static __device__ __forceinline__ S to(double v) { return (S)v; }
    template <typename S> static __device__ __forceinline__ double from(S v) { return (double)v; }
};
template <bool BF> struct CvH16 {
    typedef uint16_t Elem;
    template <typename S> static __device__ __forceinline__ S to(uint16_t v) { return (S)h16_to_f32<BF>(v); }
    // fp16: the empty asm keeps the finished fp32 value apart from its rounding.  Left to itself the compiler folds alpha * x and the
    // rounding into v_fma_mixlo/hi_f16 (alpha, x, +0), and (-0) * alpha + (+0) is +0: the sign of a zero of A was lost.
    template <typename S> static __device__ __forceinline__ uint16_t from(S v) {
        float f = (float)v;
        if constexpr (!BF) asm("" : "+v"(f));
        return f32_to_h16<BF>(f);
    }
};
typedef CvH16<true> CvBF16;
typedef CvH16<false> CvF16;

template <class KA, class KD> struct CvPair {
    typedef typename KA::Elem EA;
    typedef typename KD::Elem ED;
    static constexpr int SA = (int)sizeof(EA), SD = (int)sizeof(ED);
    static constexpr int LV = 16 / (SA < SD ? SA : SD);
    static constexpr bool NARROW = SD < SA;
    typedef typename std::conditional<(SA == 8 || SD == 8), double, float>::type S;       // compute type of the pair
};

// LV elements of storage type E at p (16 or 32 bytes, 16-byte aligned), as 16-byte accesses; NT: nontemporal (global memory)
template <typename E, int LV, bool NT>
__device__ __forceinline__ void cv_load_lane(const E* p, E (&v)[LV]) {
    constexpr int PER = 16 / (int)sizeof(E), NCH = LV / PER;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        u32x4e raw;
        if constexpr (NT) raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4e*>(p) + c);
        else raw = *(reinterpret_cast<const u32x4e*>(p) + c);
        E e[PER];
        __builtin_memcpy(e, &raw, 16);
#pragma unroll
        for (int i = 0; i < PER; ++i) v[c * PER + i] = e[i];
    }
}
template <typename E, int LV, bool NT>
__device__ __forceinline__ void cv_store_lane(E* p, const E (&v)[LV]) {
    constexpr int PER = 16 / (int)sizeof(E), NCH = LV / PER;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        E e[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) e[i] = v[c * PER + i];
        u32x4e raw;
        __builtin_memcpy(&raw, e, 16);
        if constexpr (NT) __builtin_nontemporal_store(raw, reinterpret_cast<u32x4e*>(p) + c);
        else *(reinterpret_cast<u32x4e*>(p) + c) = raw;
    }
}

template <typename S> __device__ __forceinline__ S cv_alpha(const Ew2DParams& p) { return sizeof(S) == 8 ? (S)p.alpha64 : (S)p.alpha; }
template <typename S> __device__ __forceinline__ S cv_gamma(const Ew2DParams& p) { return sizeof(S) == 8 ? (S)p.gamma64 : (S)p.gamma; }

// v = alpha * unA(v) on LV values of the compute type
template <bool UN, typename S, int LV>
__device__ __forceinline__ void cv_scale(const Ew2DParams& p, S (&v)[LV]) {
    un_apply_n<UN, S, LV>(p.unA, v);
    const S alpha = cv_alpha<S>(p);
#pragma unroll
    for (int i = 0; i < LV; ++i) v[i] = alpha * v[i];
}

// v = opAC(v, gamma * unC(C)) for the LV elements of C (D's type) that start at cp: 16-byte lanes where C is contiguous along dim0
template <class KD, bool UN, typename S, int LV>
__device__ __forceinline__ void cv_join_c(const Ew2DParams& p, const typename KD::Elem* cp, S (&v)[LV]) {
    typedef typename KD::Elem ED;
    ED raw[LV];
    if (p.sC0 == 1) {
        cv_load_lane<ED, LV, true>(cp, raw);
    } else {
#pragma unroll
        for (int i = 0; i < LV; ++i) raw[i] = cp[(int64_t)i * p.sC0];
    }
    S c[LV];
#pragma unroll
    for (int i = 0; i < LV; ++i) c[i] = KD::template to<S>(raw[i]);
    un_apply_n<UN, S, LV>(p.unC, c);
    const S gamma = cv_gamma<S>(p);
#pragma unroll
    for (int i = 0; i < LV; ++i) v[i] = ew_comb<S>(p.opAC, v[i], gamma * c[i]);
}

// ---------------------------------------------------------------------------------------------
// EW_ROWCOPY: sD0 == 1 and sA0 == 1, E0 % LV == 0, every other stride a multiple of LV, 16-byte-aligned descriptors.
// Tile = 64 lanes x LV dim0 elements x 8 dim1 rows (4 waves x 2 rows).
// ---------------------------------------------------------------------------------------------
template <class KA, class KD, bool HASC, bool UN>
__global__ void __launch_bounds__(256) ew_rowcopy_convert_kernel(const Ew2DParams p) {
    typedef CvPair<KA, KD> Pr;
    typedef typename Pr::EA EA;
    typedef typename Pr::ED ED;
    typedef typename Pr::S S;
    constexpr int LV = Pr::LV;
    const EA* A = static_cast<const EA*>(p.A);
    const ED* C = static_cast<const ED*>(p.C);
    ED*       D = static_cast<ED*>(p.D);
    (void)C;
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * (64u * LV) + (uint32_t)LV * (tid & 63);
        if (c0 >= p.E0) continue;
        EA raw[2][LV];
        uint32_t r1[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            r1[r] = t.t1 * 8u + (tid >> 6) * 2 + r;
            if (r1[r] < p.E1) cv_load_lane<EA, LV, true>(A + oA + (int64_t)r1[r] * p.sA1 + c0, raw[r]);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r1[r] >= p.E1) continue;
            S v[LV];
#pragma unroll
            for (int i = 0; i < LV; ++i) v[i] = KA::template to<S>(raw[r][i]);
            cv_scale<UN, S, LV>(p, v);
            if constexpr (HASC) cv_join_c<KD, UN, S, LV>(p, C + oC + (int64_t)r1[r] * p.sC1 + (int64_t)c0 * p.sC0, v);
            ED out[LV];
#pragma unroll
            for (int i = 0; i < LV; ++i) out[i] = KD::template from<S>(v[i]);
            cv_store_lane<ED, LV, true>(D + oD + (int64_t)r1[r] * p.sD1 + c0, out);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// EW_TRANSPOSE: sD0 == 1, sA1 == 1, E0 % LV == 0, E1 % LV == 0, every other stride a multiple of LV, 16-byte-aligned descriptors.
// ---------------------------------------------------------------------------------------------
constexpr int CV_T1 = 64;       // tile extent along dim1 (A's contiguous mode)

template <class KA, class KD, bool HASC, bool UN, int T0>
__global__ void __launch_bounds__(256) ew_transpose_convert_kernel(const Ew2DParams p) {
    typedef CvPair<KA, KD> Pr;
    typedef typename Pr::EA EA;
    typedef typename Pr::ED ED;
    typedef typename Pr::S S;
    constexpr int LV = Pr::LV;
    constexpr bool PARK_D = Pr::NARROW && !HASC;        // the LDS tile holds finished elements of D; else A's bits
    typedef typename std::conditional<PARK_D, ED, EA>::type EP;
    constexpr int T1 = CV_T1;
    constexpr int OCT = T1 / LV;                         // read: lanes along dim1
    constexpr int PCS = T0 / LV;                         // LV-element pieces of an LDS row = dim0 blocks of the tile
    constexpr int NBLK = PCS * OCT;                      // LV x LV blocks of the tile
    constexpr int RD_PASSES = (NBLK + 255) / 256;
    constexpr int RD_LANES = NBLK >= 256 ? 256 : NBLK;
    constexpr int BROWS = 256 / OCT;                     // dim0 blocks per read pass
    constexpr int LPW = PCS;                             // write: lanes per dim1 row
    constexpr int RPW = 256 / LPW;                       //        dim1 rows per pass
    constexpr int WR_PASSES = T1 / RPW;
    static_assert(PCS >= 8 && (PCS & (PCS - 1)) == 0 && T1 % RPW == 0 && NBLK % RD_LANES == 0, "tile shape");
    static_assert(T0 * T1 * (int)sizeof(EP) <= 32768, "LDS tile");
    __shared__ __attribute__((aligned(16))) EP tile[T1 * T0];   // [dim1][dim0], pieces swizzled
    const EA* A = static_cast<const EA*>(p.A);
    const ED* C = static_cast<const ED*>(p.C);
    ED*       D = static_cast<ED*>(p.D);
    (void)C;
    const int tid = threadIdx.x;
    const uint32_t nIds = p.order ? 8u * p.idsPerXcd : p.nBlocks;
    for (uint32_t b = blockIdx.x; b < nIds; b += gridDim.x) {
        TileId t;
        if (!ordered_tile(p, b, t)) continue;
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t i0 = t.t0 * T0, i1 = t.t1 * T1;
        const bool full = (i0 + T0 <= p.E0) && (i1 + T1 <= p.E1);
        // ---- read: lane -> block (dim1 block oct, dim0 block brow [+ BROWS per pass]): LV rows of LV elements
        if (tid < RD_LANES) {
            const int oct = tid % OCT, brow = tid / OCT;
            const uint32_t c1 = i1 + (uint32_t)(LV * oct);
            EA in[RD_PASSES][LV][LV];
#pragma unroll
            for (int ps = 0; ps < RD_PASSES; ++ps) {
                const uint32_t r0 = i0 + (uint32_t)(LV * (brow + BROWS * ps));
#pragma unroll
                for (int k = 0; k < LV; ++k) {
                    if (full || (c1 < p.E1 && r0 + k < p.E0)) {
                        cv_load_lane<EA, LV, true>(A + oA + (int64_t)(r0 + k) * p.sA0 + c1, in[ps][k]);
                    } else {
#pragma unroll
                        for (int j = 0; j < LV; ++j) in[ps][k][j] = EA(0);
                    }
                }
            }
#pragma unroll
            for (int ps = 0; ps < RD_PASSES; ++ps) {
                const int pc = brow + BROWS * ps;            // this block's piece of every LDS row it writes
                EP out[LV][LV];                              // [dim1 j][dim0 k]
                if constexpr (PARK_D) {
#pragma unroll
                    for (int k = 0; k < LV; ++k) {
                        S v[LV];
#pragma unroll
                        for (int j = 0; j < LV; ++j) v[j] = KA::template to<S>(in[ps][k][j]);
                        cv_scale<UN, S, LV>(p, v);
#pragma unroll
                        for (int j = 0; j < LV; ++j) out[j][k] = KD::template from<S>(v[j]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < LV; ++k)
#pragma unroll
                        for (int j = 0; j < LV; ++j) out[j][k] = in[ps][k][j];
                }
#pragma unroll
                for (int j = 0; j < LV; ++j)
                    cv_store_lane<EP, LV, false>(&tile[(LV * oct + j) * T0 + ((pc ^ (oct & 7)) * LV)], out[j]);
            }
        }
        __syncthreads();
        // ---- write: lane -> (dim0 piece tid % LPW, dim1 row tid / LPW + RPW * pass)
        {
            const int pc = tid % LPW;
            const uint32_t c0 = i0 + (uint32_t)(LV * pc);
            auto finish = [&](int lr) {
                const uint32_t r1 = i1 + (uint32_t)lr;
                EP in[LV];
                cv_load_lane<EP, LV, false>(&tile[lr * T0 + ((pc ^ ((lr / LV) & 7)) * LV)], in);
                ED out[LV];
                if constexpr (PARK_D) {
#pragma unroll
                    for (int i = 0; i < LV; ++i) out[i] = in[i];
                } else {
                    S v[LV];
#pragma unroll
                    for (int i = 0; i < LV; ++i) v[i] = KA::template to<S>(in[i]);
                    cv_scale<UN, S, LV>(p, v);
                    if constexpr (HASC) cv_join_c<KD, UN, S, LV>(p, C + oC + (int64_t)r1 * p.sC1 + (int64_t)c0 * p.sC0, v);
#pragma unroll
                    for (int i = 0; i < LV; ++i) out[i] = KD::template from<S>(v[i]);
                }
                cv_store_lane<ED, LV, true>(D + oD + (int64_t)r1 * p.sD1 + c0, out);
            };
            if (full) {
#pragma unroll
                for (int pass = 0; pass < WR_PASSES; ++pass) finish(tid / LPW + RPW * pass);
            } else if (c0 < p.E0) {
#pragma unroll 1
                for (int pass = 0; pass < WR_PASSES; ++pass) {
                    const int lr = tid / LPW + RPW * pass;
                    if (i1 + (uint32_t)lr < p.E1) finish(lr);
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// EW_GENERIC: any strides, extents and alignment.  Tile = 64 dim0 elements x 4 dim1 rows, one element per lane.
// ---------------------------------------------------------------------------------------------
template <class KA, class KD, bool HASC, bool UN>
__global__ void __launch_bounds__(256) ew_generic_convert_kernel(const Ew2DParams p) {
    typedef CvPair<KA, KD> Pr;
    typedef typename Pr::EA EA;
    typedef typename Pr::ED ED;
    typedef typename Pr::S S;
    const EA* A = static_cast<const EA*>(p.A);
    const ED* C = static_cast<const ED*>(p.C);
    ED*       D = static_cast<ED*>(p.D);
    const S alpha = cv_alpha<S>(p), gamma = cv_gamma<S>(p);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * 64u + (tid & 63);
        const uint32_t r1 = t.t1 * 4u + (tid >> 6);
        if (c0 >= p.E0 || r1 >= p.E1) continue;
        S v = alpha * un_apply<UN, S>(p.unA, KA::template to<S>(A[oA + (int64_t)c0 * p.sA0 + (int64_t)r1 * p.sA1]));
        if constexpr (HASC)
            v = ew_comb<S>(p.opAC, v, gamma * un_apply<UN, S>(p.unC, KD::template to<S>(C[oC + (int64_t)c0 * p.sC0 + (int64_t)r1 * p.sC1])));
        D[oD + (int64_t)c0 * p.sD0 + (int64_t)r1 * p.sD1] = KD::template from<S>(v);
    }
}

// ---- launchers --------------------------------------------------------------------------------
template <class KA, class KD, bool HASC, bool UN, int T0>
static hipError_t launch_cv_tile(const Ew2DParams& p, unsigned grid, hipStream_t stream) {
    typedef CvPair<KA, KD> Pr;
    constexpr int park = (Pr::NARROW && !HASC) ? Pr::SD : Pr::SA;
    if constexpr (T0 * CV_T1 * park <= 32768) {
        hipLaunchKernelGGL((ew_transpose_convert_kernel<KA, KD, HASC, UN, T0>), dim3(grid), dim3(256), 0, stream, p);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;      // (the planner never asks for a tile that 32 KiB of LDS do not hold)
    }
}

template <class KA, class KD, bool HASC, bool UN>
static hipError_t launch_cv(const Ew2DParams& p, int variant, hipStream_t stream) {
    constexpr uint32_t LV = (uint32_t)CvPair<KA, KD>::LV;
    const unsigned grid = ew_tiled_grid(p, variant);
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.D) | (HASC ? reinterpret_cast<uintptr_t>(p.C) : 0);
    if (variant == EW_TRANSPOSE) {
        if ((ptrs & 15u) != 0u || p.tile1 != (uint32_t)CV_T1 || p.E0 % LV != 0u || p.E1 % LV != 0u) return hipErrorInvalidValue;
        switch (p.tile0) {
            case 256: return launch_cv_tile<KA, KD, HASC, UN, 256>(p, grid, stream);
            case 128: return launch_cv_tile<KA, KD, HASC, UN, 128>(p, grid, stream);
            case 64:  return launch_cv_tile<KA, KD, HASC, UN, 64>(p, grid, stream);
            default:  return hipErrorInvalidValue;
        }
    }
    if (variant == EW_ROWCOPY) {
        if ((ptrs & 15u) != 0u || p.tile0 != 64u * LV || p.tile1 != 8u || p.E0 % LV != 0u) return hipErrorInvalidValue;
        hipLaunchKernelGGL((ew_rowcopy_convert_kernel<KA, KD, HASC, UN>), dim3(grid), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (variant == EW_GENERIC) {
        if (p.tile0 != 64u || p.tile1 != 4u) return hipErrorInvalidValue;
        hipLaunchKernelGGL((ew_generic_convert_kernel<KA, KD, HASC, UN>), dim3(grid), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;          // a missing kernel is an error, never another path
}

template <class KA, class KD>
static hipError_t launch_cv_pair(const Ew2DParams& p, int variant, hipStream_t stream) {
    const bool hasC = p.C != nullptr;
    const bool un = un_active(p.unA) || (hasC && un_active(p.unC));
    if (hasC) return un ? launch_cv<KA, KD, true, true>(p, variant, stream) : launch_cv<KA, KD, true, false>(p, variant, stream);
    return un ? launch_cv<KA, KD, false, true>(p, variant, stream) : launch_cv<KA, KD, false, false>(p, variant, stream);
}

hipError_t launch_elementwise_convert(const Ew2DParams& p, int variant, int dtypeA, int dtypeD, hipStream_t stream) {
    if (p.nBlocks == 0) return hipSuccess;
    if (p.E != nullptr || p.X != nullptr) return hipErrorInvalidValue;      // (planned for permutations and the binary form only)
    if (dtypeA == HIP_R_16BF && dtypeD == HIP_R_32F) return launch_cv_pair<CvBF16, CvF32>(p, variant, stream);
    if (dtypeA == HIP_R_16F && dtypeD == HIP_R_32F)  return launch_cv_pair<CvF16, CvF32>(p, variant, stream);
    if (dtypeA == HIP_R_32F && dtypeD == HIP_R_16BF) return launch_cv_pair<CvF32, CvBF16>(p, variant, stream);
    if (dtypeA == HIP_R_32F && dtypeD == HIP_R_16F)  return launch_cv_pair<CvF32, CvF16>(p, variant, stream);
    if (dtypeA == HIP_R_32F && dtypeD == HIP_R_64F)  return launch_cv_pair<CvF32, CvF64>(p, variant, stream);
    if (dtypeA == HIP_R_64F && dtypeD == HIP_R_32F)  return launch_cv_pair<CvF64, CvF32>(p, variant, stream);
    return hipErrorInvalidValue;
}

}  // namespace ctamd
