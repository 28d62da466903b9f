// elementwise_trinary_cplx.hip — cutensorElementwiseTrinaryExecute on complex64 / complex128 tensors (elementwise_trinary.cu:174-182,
// :223-227 on HIP_C_32F / HIP_C_64F data):
//
//   D = opAC(opAB(delta * cj(E), opAB(xi * cj(perm X), alpha * cj(perm A))), gamma * cj(perm C))
//
// with the operands a form of plan_elementwise_trinary attaches (E: an operand with D's strides — the one that already has D's layout, or
// D itself in the second pass of the two-pass form; X: a second permuted operand; either may be absent), cj = identity or conjugation per
// operand, opAB / opAC = ADD or MUL, complex scalars.  Arithmetic in the data's own precision on (re, im) pairs (wide_elem.h: WCplx), the
// complex product as four real products and two sums; nothing is rounded between the loads and the store.
//
// The kernels of elementwise.hip for 8- / 16-byte elements take neither E nor X, and their argument block (Ew2DParams) has no room for
// the imaginary parts of xi and delta or for the conjugation of X and E: Ew3CplxParams below wraps it.  Same tile decompositions, same
// planner conditions (plan_elementwise: a 16-byte lane holds NV = 2 complex64 / 1 complex128 elements):
//
//   ew3c_transpose_kernel   EW_TRANSPOSE: a T0 x T1 tile of A (and of X: a second LDS tile) is read with 16-byte lanes along dim1,
//                           transposed NV x NV in registers, parked in LDS as [dim1][dim0] and written with 16-byte lanes along dim0,
//                           where E and C join.  128 x 32 (complex64) / 64 x 32 (complex128): 1-KiB written row segments.  With X
//                           complex64 takes 64 x 64 tiles — tile0 halved: 512-B segments on the two strided reads and on the write,
//                           and two tiles of 64 x (64 + 2) x 8 bytes are the real two-tile form's 67584 bytes of LDS exactly;
//                           complex128 keeps 64 x 32 (2 x 33280 bytes).
//   ew3c_rowcopy_kernel     EW_ROWCOPY: A and D share the stride-1 mode; 64 lanes x NV elements x 8 dim1 rows, no LDS.
//   ew3c_generic_kernel     EW_GENERIC: any strides and alignment, one element per lane, lanes along dim0 — A, X, E and C.
//
// E is always read with 16-byte lanes in the tiled kernels (it has D's strides), C where it is contiguous along dim0 and element by
// element otherwise.  Every row of C / E a lane combines with — and every row of A / X it parks — is requested before the first one is
// used.  HBM-bound: 4 |D| bytes (A or X, E or X, C, D).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elementwise_common.h"
#include "launch.h"
#include "params.h"
#include "wide_elem.h"

namespace ctamd {

// Ew2DParams as the planner filled it, and what a complex trinary launch needs beside it: alpha64 / alphaIm, gamma64 / gammaIm, xi64 and
// delta64 hold the scalars' parts that have a field there, conjA / conjC the conjugation of the tile operand and of C
struct Ew3CplxParams {
    Ew2DParams p;
    double     xiIm, deltaIm;      // imaginary parts of xi (X's scalar) and delta (E's scalar)
    int32_t    conjX, conjE;
};

// v = alpha * a, then X, E and C join in that order (the order of the real kernels, elementwise_kernels.inc)
template <class Tr, bool HASX>
__device__ __forceinline__ typename Tr::Acc c3_finish(const Ew3CplxParams& q, typename Tr::Acc a, typename Tr::Acc x, typename Tr::Acc e, bool hasE,
                                                      typename Tr::Acc c, bool hasC) {
    const Ew2DParams& p = q.p;
    typename Tr::Acc v = Tr::scale(p.alpha64, p.alphaIm, a);
    if constexpr (HASX) v = Tr::apply(p.opAB, Tr::scale(p.xi64, q.xiIm, x), v);
    if (hasE) v = Tr::apply(p.opAB, Tr::scale(p.delta64, q.deltaIm, e), v);
    if (hasC) v = Tr::apply(p.opAC, v, Tr::scale(p.gamma64, p.gammaIm, c));
    return v;
}

// the NV elements of C a lane combines with, as one 16-byte unit: a 16-byte load where C is contiguous along dim0, else element by element
template <class Tr>
__device__ __forceinline__ wu32x4 c3_load_c(const typename Tr::Elem* cp, int64_t sC0) {
    if (sC0 == 1) return __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(cp));
    typename Tr::Acc t[Tr::NV];
#pragma unroll
    for (int e = 0; e < Tr::NV; ++e) t[e] = Tr::load1(cp + (int64_t)e * sC0, false);
    return Tr::pack(t);
}

template <class Tr, int T0, int T1, bool HASX>
__global__ void __launch_bounds__(256) ew3c_transpose_kernel(const Ew3CplxParams q) {
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    constexpr int NV = Tr::NV;
    constexpr int LD = T0 + NV;                     // LDS row stride (elements)
    constexpr int LPR = T1 / NV;                    // read: lanes per dim0 row
    constexpr int RPP = (256 / LPR) * NV;           //       dim0 rows per pass
    constexpr int RD_PASSES = T0 / RPP;
    constexpr int LPW = T0 / NV;                    // write: lanes per dim1 row
    constexpr int RPW = 256 / LPW;                  //        dim1 rows per pass
    constexpr int WR_PASSES = T1 / RPW;
    static_assert(T0 % RPP == 0 && T1 % RPW == 0 && 256 % LPR == 0 && 256 % LPW == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) Elem tile[T1 * LD];                  // [dim1][dim0]
    __shared__ __attribute__((aligned(16))) Elem tileX[HASX ? T1 * LD : NV];
    const Ew2DParams& p = q.p;
    const Elem* A = static_cast<const Elem*>(p.A);
    const Elem* X = static_cast<const Elem*>(p.X);
    const Elem* C = static_cast<const Elem*>(p.C);
    const Elem* E = static_cast<const Elem*>(p.E);
    Elem*       D = static_cast<Elem*>(p.D);
    const int tid = threadIdx.x;
    const bool conjA = p.conjA != 0, conjX = q.conjX != 0, conjE = q.conjE != 0, conjC = p.conjC != 0;
    const uint32_t nIds = p.order ? 8u * p.idsPerXcd : p.nBlocks;
    for (uint32_t b = blockIdx.x; b < nIds; b += gridDim.x) {
        TileId t;
        if (!ordered_tile(p, b, t)) continue;
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t i0 = t.t0 * T0, i1 = t.t1 * T1;
        const bool full = (i0 + T0 <= p.E0) && (i1 + T1 <= p.E1);
        {   // ---- read: lane -> (dim1 unit c1 = tid % LPR, dim0 rows r0 .. r0 + NV - 1), RD_PASSES passes; A's and X's rows all in flight
            const int      l1 = NV * (tid % LPR);
            const uint32_t c1 = i1 + l1;
            wu32x4 in[RD_PASSES][NV], inX[HASX ? RD_PASSES : 1][NV];
#pragma unroll
            for (int ps = 0; ps < RD_PASSES; ++ps) {
                const uint32_t r0 = i0 + NV * (tid / LPR) + RPP * ps;
#pragma unroll
                for (int r = 0; r < NV; ++r) {
                    in[ps][r] = wu32x4{0u, 0u, 0u, 0u};
                    if (full || (c1 < p.E1 && (r0 + r) < p.E0))
                        in[ps][r] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(A + oA + (int64_t)(r0 + r) * p.sA0 + c1));
                }
            }
            if constexpr (HASX) {
                const int64_t oX = rest_offset_x(p.rest, p.restX, t.rest);
#pragma unroll
                for (int ps = 0; ps < RD_PASSES; ++ps) {
                    const uint32_t r0 = i0 + NV * (tid / LPR) + RPP * ps;
#pragma unroll
                    for (int r = 0; r < NV; ++r) {
                        inX[ps][r] = wu32x4{0u, 0u, 0u, 0u};
                        if (full || (c1 < p.E1 && (r0 + r) < p.E0))
                            inX[ps][r] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(X + oX + (int64_t)(r0 + r) * p.sX0 + c1));
                    }
                }
            }
#pragma unroll
            for (int ps = 0; ps < RD_PASSES; ++ps) {
                const int l0 = NV * (tid / LPR) + RPP * ps;
                // NV x NV register transpose: unit j of the output = element j of every input row
                Acc v[NV][NV];
#pragma unroll
                for (int r = 0; r < NV; ++r) Tr::unpack(in[ps][r], v[r], conjA);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    Acc o[NV];
#pragma unroll
                    for (int r = 0; r < NV; ++r) o[r] = v[r][j];
                    *reinterpret_cast<wu32x4*>(&tile[(l1 + j) * LD + l0]) = Tr::pack(o);
                }
                if constexpr (HASX) {
#pragma unroll
                    for (int r = 0; r < NV; ++r) Tr::unpack(inX[ps][r], v[r], conjX);
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        Acc o[NV];
#pragma unroll
                        for (int r = 0; r < NV; ++r) o[r] = v[r][j];
                        *reinterpret_cast<wu32x4*>(&tileX[(l1 + j) * LD + l0]) = Tr::pack(o);
                    }
                }
            }
        }
        __syncthreads();
        {   // ---- write: lane -> (dim0 unit c0 = tid % LPW, dim1 row tid / LPW + RPW * pass); the rows of C and E of ALL passes are
            // requested before the first one is used
            const int      l0 = NV * (tid % LPW);
            const uint32_t c0 = i0 + l0;
            wu32x4 cv[WR_PASSES], ev[WR_PASSES];
#pragma unroll
            for (int pass = 0; pass < WR_PASSES; ++pass) {
                const uint32_t r1 = i1 + tid / LPW + RPW * pass;
                const bool ok = full || (c0 < p.E0 && r1 < p.E1);
                cv[pass] = wu32x4{0u, 0u, 0u, 0u};
                ev[pass] = wu32x4{0u, 0u, 0u, 0u};
                if (ok && C != nullptr) cv[pass] = c3_load_c<Tr>(C + oC + (int64_t)r1 * p.sC1 + (int64_t)c0 * p.sC0, p.sC0);
                if (ok && E != nullptr) ev[pass] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(E + oD + (int64_t)r1 * p.sD1 + c0));
            }
#pragma unroll
            for (int pass = 0; pass < WR_PASSES; ++pass) {
                const int      lr = tid / LPW + RPW * pass;
                const uint32_t r1 = i1 + lr;
                if (full || (c0 < p.E0 && r1 < p.E1)) {
                    Acc v[NV], x[NV], e[NV], c[NV];
                    Tr::unpack(*reinterpret_cast<const wu32x4*>(&tile[lr * LD + l0]), v, false);
                    if constexpr (HASX) Tr::unpack(*reinterpret_cast<const wu32x4*>(&tileX[lr * LD + l0]), x, false);
                    Tr::unpack(ev[pass], e, conjE);
                    Tr::unpack(cv[pass], c, conjC);
#pragma unroll
                    for (int k = 0; k < NV; ++k) v[k] = c3_finish<Tr, HASX>(q, v[k], HASX ? x[k] : v[k], e[k], E != nullptr, c[k], C != nullptr);
                    __builtin_nontemporal_store(Tr::pack(v), reinterpret_cast<wu32x4*>(D + oD + (int64_t)r1 * p.sD1 + c0));
                }
            }
        }
        __syncthreads();
    }
}

// row copy: A and D share the stride-1 mode — tile = 64 lanes x NV dim0 elements x 8 dim1 rows (4 waves x 2 rows), no LDS
template <class Tr>
__global__ void __launch_bounds__(256) ew3c_rowcopy_kernel(const Ew3CplxParams q) {
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    constexpr int NV = Tr::NV;
    const Ew2DParams& p = q.p;
    const Elem* A = static_cast<const Elem*>(p.A);
    const Elem* C = static_cast<const Elem*>(p.C);
    const Elem* E = static_cast<const Elem*>(p.E);
    Elem*       D = static_cast<Elem*>(p.D);
    const int tid = threadIdx.x;
    const bool conjA = p.conjA != 0, conjE = q.conjE != 0, conjC = p.conjC != 0;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * (64u * NV) + (uint32_t)NV * (tid & 63);
        if (c0 >= p.E0) continue;
        wu32x4 raw[2], cv[2], ev[2];
        uint32_t r1[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            r1[r] = t.t1 * 8u + (tid >> 6) * 2 + r;
            raw[r] = cv[r] = ev[r] = wu32x4{0u, 0u, 0u, 0u};
            if (r1[r] < p.E1) {
                raw[r] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(A + oA + (int64_t)r1[r] * p.sA1 + c0));
                if (E != nullptr) ev[r] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(E + oD + (int64_t)r1[r] * p.sD1 + c0));
                if (C != nullptr) cv[r] = c3_load_c<Tr>(C + oC + (int64_t)r1[r] * p.sC1 + (int64_t)c0 * p.sC0, p.sC0);
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r1[r] >= p.E1) continue;
            Acc v[NV], e[NV], c[NV];
            Tr::unpack(raw[r], v, conjA);
            Tr::unpack(ev[r], e, conjE);
            Tr::unpack(cv[r], c, conjC);
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = c3_finish<Tr, false>(q, v[k], v[k], e[k], E != nullptr, c[k], C != nullptr);
            __builtin_nontemporal_store(Tr::pack(v), reinterpret_cast<wu32x4*>(D + oD + (int64_t)r1[r] * p.sD1 + c0));
        }
    }
}

// element gather: one (re, im) pair per lane, 64 dim0 elements x 4 dim1 rows per workgroup (ew_generic_cplx_kernel's decomposition); the
// single launch of the two-pass form whose C overlaps D runs here too — a lane reads its element of C before it writes that element of D
template <class Tr>
__global__ void __launch_bounds__(256) ew3c_generic_kernel(const Ew3CplxParams q) {
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    const Ew2DParams& p = q.p;
    const Elem* A = static_cast<const Elem*>(p.A);
    const Elem* X = static_cast<const Elem*>(p.X);
    const Elem* C = static_cast<const Elem*>(p.C);
    const Elem* E = static_cast<const Elem*>(p.E);
    Elem*       D = static_cast<Elem*>(p.D);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * 64u + (tid & 63);
        const uint32_t r1 = t.t1 * 4u + (tid >> 6);
        if (c0 >= p.E0 || r1 >= p.E1) continue;
        const int64_t offD = oD + (int64_t)c0 * p.sD0 + (int64_t)r1 * p.sD1;
        Acc a = Tr::load1(A + oA + (int64_t)c0 * p.sA0 + (int64_t)r1 * p.sA1, p.conjA != 0);
        Acc x = a, e = a, c = a;
        if (X != nullptr) x = Tr::load1(X + rest_offset_x(p.rest, p.restX, t.rest) + (int64_t)c0 * p.sX0 + (int64_t)r1 * p.sX1, q.conjX != 0);
        if (E != nullptr) e = Tr::load1(E + offD, q.conjE != 0);
        if (C != nullptr) c = Tr::load1(C + oC + (int64_t)c0 * p.sC0 + (int64_t)r1 * p.sC1, p.conjC != 0);
        Acc v = Tr::scale(p.alpha64, p.alphaIm, a);
        if (X != nullptr) v = Tr::apply(p.opAB, Tr::scale(p.xi64, q.xiIm, x), v);
        if (E != nullptr) v = Tr::apply(p.opAB, Tr::scale(p.delta64, q.deltaIm, e), v);
        if (C != nullptr) v = Tr::apply(p.opAC, v, Tr::scale(p.gamma64, p.gammaIm, c));
        Tr::store1(D + offD, v);
    }
}

// T0 x T1: the transposing tile without X; TX0 x TX1: with X (the planner's tile0 / tile1 for either form)
template <class Tr, int T0, int T1, int TX0, int TX1>
static hipError_t launch_c3(const Ew3CplxParams& q, int variant, hipStream_t stream) {
    const Ew2DParams& p = q.p;
    const unsigned grid = ew_tiled_grid(p, variant);
    if (variant == EW_TRANSPOSE || variant == EW_ROWCOPY) {
        // 16-byte lanes: what the planner derived from the descriptors' alignments is checked on the pointers once more
        uintptr_t bits = reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.D) | reinterpret_cast<uintptr_t>(p.E) |
                         reinterpret_cast<uintptr_t>(p.X) | reinterpret_cast<uintptr_t>(p.C);
        if ((bits & 15u) != 0u) return hipErrorInvalidValue;
        const uint32_t t0 = variant == EW_ROWCOPY ? 64u * Tr::NV : p.X != nullptr ? (uint32_t)TX0 : (uint32_t)T0;
        if (p.tile0 != t0 || (variant == EW_TRANSPOSE && p.tile1 != (p.X != nullptr ? (uint32_t)TX1 : (uint32_t)T1))) return hipErrorInvalidValue;
    }
    if (variant == EW_TRANSPOSE) {
        if (p.X != nullptr) hipLaunchKernelGGL((ew3c_transpose_kernel<Tr, TX0, TX1, true>), dim3(grid), dim3(256), 0, stream, q);
        else                hipLaunchKernelGGL((ew3c_transpose_kernel<Tr, T0, T1, false>), dim3(grid), dim3(256), 0, stream, q);
    } else if (variant == EW_ROWCOPY) {
        if (p.X != nullptr) return hipErrorInvalidValue;          // (the planner gives a second permuted operand the transposing or the gather kernel)
        hipLaunchKernelGGL(ew3c_rowcopy_kernel<Tr>, dim3(grid), dim3(256), 0, stream, q);
    } else if (variant == EW_GENERIC) {
        if (p.tile0 != 64u || p.tile1 != 4u) return hipErrorInvalidValue;
        hipLaunchKernelGGL(ew3c_generic_kernel<Tr>, dim3(grid), dim3(256), 0, stream, q);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_elementwise_trinary_cplx(const Ew2DParams& p, const Ew3CplxExtras& x, int variant, int dtype, hipStream_t stream) {
    if (p.nBlocks == 0) return hipSuccess;
    if (p.unA != 0 || p.unX != 0 || p.unE != 0 || p.unC != 0) return hipErrorInvalidValue;   // (complex data takes IDENTITY and CONJ only)
    const Ew3CplxParams q{p, x.xiIm, x.deltaIm, x.conjX, x.conjE};
    if (dtype == HIP_C_32F) return launch_c3<WCplx<float>, 128, 32, 64, 64>(q, variant, stream);
    if (dtype == HIP_C_64F) return launch_c3<WCplx<double>, 64, 32, 64, 32>(q, variant, stream);
    return hipErrorInvalidValue;
}

}  // namespace ctamd
