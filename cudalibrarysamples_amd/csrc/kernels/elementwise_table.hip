// elementwise_table.hip — element-wise operations and reductions on tensors of up to 64 modes, gfx950.
//
// The kernels of elementwise.hip and reduce.hip describe a problem as two tile modes plus a "rest" index of at most four digits
// (Ew2DParams / ReduceParams); a permutation, a binary operation or a reduction whose modes do not fuse that far — the 2 x 2 x ... x 2
// state tensors of quantum-circuit and tensor-network codes, which cutensorContract already serves — is planned onto the kernels
// below instead (host/plan_elementwise_table.cpp), which read a table of up to 64 modes out of their own argument block
// (ew_table_layout.h: the block, and every piece of index arithmetic, shared with the planner and with a host harness).
//
//   D = opAC(alpha * op(perm(A)), gamma * op(perm(C)))          all six data types, op as in unary_op.h / CONJ on complex data
//
//   ew_table_tile_kernel     A and D each have a stride-1 mode and A carries every mode of D.  A tile is the union of D's leading modes and
//                            A's leading modes, each set taken by ascending stride until it spans 256 bytes (less when the union outgrows
//                            the LDS budget: 16 KiB, at most 2048 positions; more while a tile that fits has slots to spare); a mode too
//                            long for the tile is cut, its last piece partial.
//                            A workgroup builds the tile-relative offsets of its 8 (4) positions per thread ONCE, in registers, then loops
//                            over tiles: outer index decoded once per tile (wave-uniform: scalar loads and scalar arithmetic), the tile read
//                            in A's order — consecutive lanes, consecutive addresses of A — parked in LDS (ewt_slot), and written in D's
//                            order with the operators, the scalars and the C term applied on the way out.  C is read in D's order through its
//                            own strides, so a C in another mode order stays on this kernel.  Element-wise loads and stores: a run along a
//                            stride-1 mode may be two elements long.
//   ew_table_gather_kernel   everything else (a mode of D that A lacks, no stride-1 mode on a side, tile offsets beyond 32 bits): one
//                            output element per lane per step, every digit decoded, 64-bit offsets.
//   reduce_table_kernel      D[kept] = alpha * reduce_red A[kept, red] + beta * C[kept]: a lane per kept element in D's order; the offsets
//                            of the next 256 reduced elements are decoded once per workgroup, one per thread, into LDS, and every lane
//                            walks that list (a broadcast read per element, no division per step).  The reduced range is split over
//                            blockIdx.y as in reduce.hip, partials [splitR][kept] of the accumulator type, folded by
//                            reduce_table_finalize_kernel (the fold of reduce.hip decodes a kept element with four digits).
// The table is read through the kernel-argument pointer (constant address space): a run-time index into a by-value argument would
// have the compiler copy the struct into scratch.  tests/test_many_modes_resources.py keeps that honest: no private segment, no spill.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ew_table_layout.h"
#include "launch.h"
#include "params.h"
#include "unary_op.h"
#include "wide_elem.h"

namespace ctamd {

typedef const __attribute__((address_space(4))) EwTable* EwTabArgs;
__device__ __forceinline__ EwTabArgs ewt_args() { return (EwTabArgs)__builtin_amdgcn_kernarg_segment_ptr(); }

// scalars and operators of a launch, read from the argument block once
struct EwtScalars {
    double alphaRe, alphaIm, gammaRe, gammaIm;
    int32_t opAC, unA, unC;
    bool conjA, conjC;
};
__device__ __forceinline__ EwtScalars ewt_scalars(EwTabArgs tab) {
    return EwtScalars{tab->alpha64, tab->alphaIm, tab->gamma64, tab->gammaIm, tab->opAC, (int32_t)tab->unA, (int32_t)tab->unC,
                      tab->conjA != 0, tab->conjC != 0};
}
// a = the element of A as loaded (conjugated already): operator, scalar, the C term, the store
template <class Tr, bool UN>
__device__ __forceinline__ void ewt_finish(const EwtScalars& s, typename Tr::Acc a, const typename Tr::Elem* cp, typename Tr::Elem* dp) {
    typename Tr::Acc v = Tr::scale(s.alphaRe, s.alphaIm, w_un<Tr, UN>(s.unA, a));
    if (cp != nullptr) v = Tr::apply(s.opAC, v, Tr::scale(s.gammaRe, s.gammaIm, w_un<Tr, UN>(s.unC, Tr::load1(cp, Tr::CX && s.conjC))));
    Tr::store1(dp, v);
}

// an element as the tile kernel moves it from A into LDS: its bytes, whatever they mean
template <int BYTES> struct EwtRaw;
template <> struct EwtRaw<2> { typedef uint16_t type; };
template <> struct EwtRaw<4> { typedef uint32_t type; };
template <> struct EwtRaw<8> { typedef uint64_t type; };
template <> struct EwtRaw<16> { typedef wu32x4 type; };

// (256 threads, four waves per SIMD: 128 registers a lane — four workgroups a CU, whose LDS is at most 4 x 16 KiB)
template <class Tr, bool UN>
__global__ void __launch_bounds__(kEwTableThreads, 4) ew_table_tile_kernel(const EwTable) {
    typedef typename Tr::Elem Elem;
    typedef typename EwtRaw<sizeof(Elem)>::type Raw;
    constexpr uint32_t POS = ew_table_positions(sizeof(Elem)), PPT = POS / kEwTableThreads;
    __shared__ Raw park[POS];
    const EwTabArgs tab = ewt_args();
    const uint32_t tid = threadIdx.x, tilePos = tab->tilePos, tiles = tab->total;
    // tile-relative offsets do not depend on the tile: position tid + 256 j in A's order (the read) and in D's order (the write)
    uint32_t relA[PPT], cutA[PPT], relD[PPT], relC[PPT], from[PPT];      // from: LDS slot | cut digits << 12
#pragma unroll
    for (uint32_t j = 0; j < PPT; ++j) {
        const uint32_t r = tid + kEwTableThreads * j;
        const EwtPosA a = ewt_pos_a(tab, r);
        const EwtPosD d = ewt_pos_d(tab, r);
        relA[j] = a.relA; cutA[j] = a.cuts;
        relD[j] = d.relD; relC[j] = d.relC; from[j] = ewt_slot(d.rankA) | (d.cuts << 12);
    }
    const EwtScalars s = ewt_scalars(tab);
    const Elem* const A0 = static_cast<const Elem*>(tab->A);
    const Elem* const C0 = static_cast<const Elem*>(tab->C);
    Elem* const D0 = static_cast<Elem*>(tab->D);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const EwtOrigin o = ewt_tile_origin(tab, t);
        const Raw* const A = reinterpret_cast<const Raw*>(A0 + o.oA);
        Raw v[PPT];
#pragma unroll
        for (uint32_t j = 0; j < PPT; ++j)
            if (tid + kEwTableThreads * j < tilePos && ewt_live(cutA[j], o.live0, o.live1)) v[j] = A[relA[j]];
#pragma unroll
        for (uint32_t j = 0; j < PPT; ++j)
            if (tid + kEwTableThreads * j < tilePos && ewt_live(cutA[j], o.live0, o.live1)) park[ewt_slot(tid + kEwTableThreads * j)] = v[j];
        __syncthreads();
        const Elem* const C = C0 != nullptr ? C0 + o.oC : nullptr;
        Elem* const D = D0 + o.oD;
#pragma unroll
        for (uint32_t j = 0; j < PPT; ++j)
            if (tid + kEwTableThreads * j < tilePos && ewt_live(from[j] >> 12, o.live0, o.live1))
                ewt_finish<Tr, UN>(s, Tr::load1(reinterpret_cast<const Elem*>(&park[from[j] & 4095u]), Tr::CX && s.conjA), C != nullptr ? C + relC[j] : nullptr, D + relD[j]);
        __syncthreads();       // the next tile overwrites the parked one
    }
}

template <class Tr, bool UN>
__global__ void __launch_bounds__(kEwTableThreads) ew_table_gather_kernel(const EwTable) {
    typedef typename Tr::Elem Elem;
    const EwTabArgs tab = ewt_args();
    const uint32_t total = tab->total, n = tab->nEntries;
    const EwtScalars s = ewt_scalars(tab);
    const Elem* const A = static_cast<const Elem*>(tab->A);
    const Elem* const C = static_cast<const Elem*>(tab->C);
    Elem* const D = static_cast<Elem*>(tab->D);
    const uint64_t step = (uint64_t)gridDim.x * kEwTableThreads;
    for (uint64_t idx = (uint64_t)blockIdx.x * kEwTableThreads + threadIdx.x; idx < total; idx += step) {
        const EwtOffsets o = ewt_offsets(tab, 0u, n, (uint32_t)idx);
        ewt_finish<Tr, UN>(s, Tr::load1(A + o.oA, Tr::CX && s.conjA), C != nullptr ? C + o.oC : nullptr, D + o.oD);
    }
}

// D[k] = alpha * acc + beta * unC(C[k]) of a reduction (tab->gamma64 / gammaIm hold beta; C null: beta == 0)
template <class Tr, bool UN>
__device__ __forceinline__ void rdt_finish(EwTabArgs tab, const EwtOffsets& ko, typename Tr::Acc acc) {
    typedef typename Tr::Elem Elem;
    typename Tr::Acc val = Tr::scale(tab->alpha64, tab->alphaIm, acc);
    const Elem* const C = static_cast<const Elem*>(tab->C);
    if (C != nullptr)
        val = Tr::apply(W_OP_ADD, val, Tr::scale(tab->gamma64, tab->gammaIm, w_un<Tr, UN>((int32_t)tab->unC, Tr::load1(C + ko.oC, Tr::CX && tab->conjC != 0))));
    Tr::store1(static_cast<Elem*>(tab->D) + ko.oD, val);
}

template <class Tr, bool UN>
__global__ void __launch_bounds__(kEwTableThreads) reduce_table_kernel(const EwTable) {
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    __shared__ int64_t offs[kEwTableThreads];
    const EwTabArgs tab = ewt_args();
    const uint32_t tid = threadIdx.x, kept = tab->total, nKept = tab->nKept, nRed = tab->nRed;
    const uint32_t k = blockIdx.x * kEwTableThreads + tid;
    const bool live = k < kept;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * tab->redPerSplit;
    uint32_t rEnd = rBegin + tab->redPerSplit;
    if (rEnd > tab->redTotal) rEnd = tab->redTotal;
    const int op = tab->opReduce;
    const int32_t unA = (int32_t)tab->unA;
    const bool conjA = Tr::CX && tab->conjA != 0;
    const EwtOffsets ko = ewt_offsets(tab, 0u, nKept, live ? k : 0u);
    const Elem* const A = static_cast<const Elem*>(tab->A) + ko.oA;
    Acc acc = Tr::identity(op);
    for (uint32_t base = rBegin; base < rEnd; base += kEwTableThreads) {
        const uint32_t n = rEnd - base < (uint32_t)kEwTableThreads ? rEnd - base : (uint32_t)kEwTableThreads;
        __syncthreads();                                       // (the previous list has been walked)
        if (tid < n) offs[tid] = ewt_offsets(tab, nKept, nRed, base + tid).oA;
        __syncthreads();
        if (!live) continue;
        uint32_t i = 0;
        for (; i + 4u <= n; i += 4u) {                         // four loads in flight; the combines stay in index order
            Acc x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = Tr::load1(A + offs[i + (uint32_t)u], conjA);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = Tr::apply(op, acc, w_un<Tr, UN>(unA, x[u]));
        }
        for (; i < n; ++i) acc = Tr::apply(op, acc, w_un<Tr, UN>(unA, Tr::load1(A + offs[i], conjA)));
    }
    if (!live) return;
    if (tab->partial != nullptr) {
        static_cast<Acc*>(tab->partial)[(size_t)split * kept + k] = acc;
        return;
    }
    rdt_finish<Tr, UN>(tab, ko, acc);
}

// D[k] = alpha * combine_s partial[s][k] + beta * unC(C[k])      (the partials already hold unA(A))
template <class Tr, bool UN>
__global__ void __launch_bounds__(kEwTableThreads) reduce_table_finalize_kernel(const EwTable) {
    typedef typename Tr::Acc Acc;
    const EwTabArgs tab = ewt_args();
    const uint32_t kept = tab->total;
    const uint32_t k = blockIdx.x * kEwTableThreads + threadIdx.x;
    if (k >= kept) return;
    const int op = tab->opReduce;
    const Acc* const P = static_cast<const Acc*>(tab->partial) + k;
    Acc acc = Tr::identity(op);
    const uint32_t splitR = tab->splitR;
    for (uint32_t sp = 0; sp < splitR; ++sp) acc = Tr::apply(op, acc, P[(size_t)sp * kept]);
    rdt_finish<Tr, UN>(tab, ewt_offsets(tab, 0u, tab->nKept, k), acc);
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
// KERNEL<traits of the data type, UN>: the identity twin, or the operator twin when an operand this launch reads carries a unary operator
#define CTAMD_EWT_REAL(KERNEL, TR, grid)                                                                          \
    do {                                                                                                          \
        if (un) hipLaunchKernelGGL((KERNEL<TR, true>), grid, dim3(kEwTableThreads), 0, stream, t);                \
        else    hipLaunchKernelGGL((KERNEL<TR, false>), grid, dim3(kEwTableThreads), 0, stream, t);               \
    } while (0)
#define CTAMD_EWT_CPLX(KERNEL, TR, grid)                                                                          \
    do {                                                                                                          \
        if (un) return hipErrorInvalidValue;               /* (the planner admits unary operators on real data only) */ \
        hipLaunchKernelGGL((KERNEL<TR, false>), grid, dim3(kEwTableThreads), 0, stream, t);                       \
    } while (0)
#define CTAMD_EWT_BY_TYPE(KERNEL, grid, F32)                                                                      \
    switch (dtype) {                                                                                              \
        case HIP_R_32F:  CTAMD_EWT_REAL(KERNEL, F32, grid); break;                                                \
        case HIP_R_64F:  CTAMD_EWT_REAL(KERNEL, WF64, grid); break;                                               \
        case HIP_R_16F:  CTAMD_EWT_REAL(KERNEL, WH16<false>, grid); break;                                        \
        case HIP_R_16BF: CTAMD_EWT_REAL(KERNEL, WH16<true>, grid); break;                                         \
        case HIP_C_32F:  CTAMD_EWT_CPLX(KERNEL, WCplx<float>, grid); break;                                       \
        case HIP_C_64F:  CTAMD_EWT_CPLX(KERNEL, WCplx<double>, grid); break;                                      \
        default: return hipErrorInvalidValue;                                                                     \
    }

hipError_t launch_elementwise_table(const EwTable& t, int dtype, unsigned grid, hipStream_t stream) {
    if (t.total == 0 || grid == 0) return hipSuccess;
    const bool un = un_active(t.unA) || (t.C != nullptr && un_active(t.unC));
    if (t.kind == EWT_TILE) {
        CTAMD_EWT_BY_TYPE(ew_table_tile_kernel, dim3(grid), WF32<float>)
    } else if (t.kind == EWT_GATHER) {
        CTAMD_EWT_BY_TYPE(ew_table_gather_kernel, dim3(grid), WF32<float>)
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_reduce_table(const EwTable& t, int dtype, bool acc64, hipStream_t stream) {
    if (t.total == 0) return hipSuccess;
    if (t.kind != EWT_REDUCE || (t.splitR > 1 && t.partial == nullptr)) return hipErrorInvalidValue;
    const unsigned blocks = (t.total + kEwTableThreads - 1u) / kEwTableThreads;
    {   // the operator twin: A carries a unary operator, or C does and this launch is the one that reads C
        const bool un = un_active(t.unA) || (t.partial == nullptr && t.C != nullptr && un_active(t.unC));
        const dim3 grid(blocks, t.splitR);
        if (acc64) { CTAMD_EWT_BY_TYPE(reduce_table_kernel, grid, WF32<double>) }
        else       { CTAMD_EWT_BY_TYPE(reduce_table_kernel, grid, WF32<float>) }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || t.partial == nullptr) return e;
    const bool un = t.C != nullptr && un_active(t.unC);           // (unA went into the partials)
    if (acc64) { CTAMD_EWT_BY_TYPE(reduce_table_finalize_kernel, dim3(blocks), WF32<double>) }
    else       { CTAMD_EWT_BY_TYPE(reduce_table_finalize_kernel, dim3(blocks), WF32<float>) }
    return hipGetLastError();
}

}  // namespace ctamd
