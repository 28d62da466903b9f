// reduce.hip — HBM-bound tensor reduction kernels for gfx950.
//
// Replaces the closed kernels behind cutensorReduce (reference call sites:
// cuTENSOR/reduction.cu:219-222 "C_{m,v} = alpha * sum_{h,k} A_{m,h,k,v} + beta * C_{m,v}" :49-61,
// and cuTENSOR/einsum.cu:369-372).
//
// The planner splits A's modes into kept modes (they appear in D) and reduced modes, each a
// mixed-radix group (params.h).  Roofline: HBM; algorithmic bytes = |A| + |D| (+ |C| iff beta != 0),
// reduction.cu:229-231.
//
//   RED_COL      A's stride-1 mode is kept.  One lane owns 4 consecutive kept elements (float4),
//                walks its share of the reduced index space and keeps 4 running values.  Wave
//                loads are 1 KiB contiguous.
//   RED_ROW      A's stride-1 mode is reduced.  One wave owns one kept element, its lanes stride
//                over the reduced space with float4 loads and combine through DPP shuffles.
//   RED_GENERIC  any strides / dtype: one lane per kept element, scalar gathers.
//
// When the kept space alone cannot fill 256 CUs the reduced range is split across workgroups
// (splitR) into a [splitR][kept] partial buffer in the caller's workspace and folded by
// reduce_finalize_kernel, which also applies alpha / beta.
//
// The kernels of real data are in reduce_kernels.inc, included twice below: as x_kernel (the identity twins) and as x_un_kernel.
// Unary operators on real data (unary_op.h; UN = true, the operator twin of each kernel): unA on every element of A as it is loaded —
// never on the accumulators' identity element, never on a partial — and unC on C where beta * C joins: the kernel's last step without a
// split, reduce_finalize_kernel with one.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "launch.h"
#include "params.h"
#include "unary_op.h"
#include "wide_elem.h"

namespace ctamd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { OP_ADD = 3, OP_MUL = 5, OP_MAX = 6, OP_MIN = 7 };   // cutensorOperator_t values

template <typename S> __device__ __forceinline__ S red_identity(int op) {
    switch (op) {
        case OP_MUL: return (S)1;
        case OP_MAX: return -(S)INFINITY;
        case OP_MIN: return (S)INFINITY;
        default: return (S)0;
    }
}
template <typename S> __device__ __forceinline__ S red_apply(int op, S a, S b) {
    switch (op) {
        case OP_MUL: return a * b;
        case OP_MAX: return a > b ? a : b;
        case OP_MIN: return a < b ? a : b;
        default: return a + b;
    }
}

__device__ __forceinline__ uint32_t rd_fast_div(uint32_t n, const FastDiv& d) {
    return __umulhi(n, d.magic) >> d.shift;
}
template <int SLOT>
__device__ __forceinline__ int64_t rd_offset(const ModeGroup& g, uint32_t idx) {
    // fixed trip count, branch-free: padding modes are {d = 1, magic = 0, stride = 0}
    int64_t off = 0;
#pragma unroll
    for (int i = 0; i < kMaxGroupModes; ++i) {
        const uint32_t q = rd_fast_div(idx, g.div[i]);
        off += (int64_t)(idx - q * g.div[i].d) * g.stride[SLOT][i];
        idx = q;
    }
    return off;
}

// ---------------------------------------------------------------------------------------------
// RED_COL / RED_ROW for every other element type (round 6; wide_elem.h): fp64, complex64, complex128 in the data's own precision,
// bf16 / fp16 with fp32 accumulation.  The fp32 kernels above, with a 16-byte lane = Tr::NV elements (2 / 2 / 1 / 8) and the
// arithmetic of the traits class: ADD / MUL / MAX / MIN on real data, ADD / MUL with conjugation of A on complex data.  Partials are
// [splitR][kept] values of the accumulator type — what reduce_finalize_kernel / reduce_finalize_cplx_kernel fold.
// ---------------------------------------------------------------------------------------------
template <class Tr, bool UN>
__device__ __forceinline__ void w_finish(const ReduceParams& p, uint32_t k, typename Tr::Acc acc) {
    typedef typename Tr::Elem Elem;
    typename Tr::Acc val = Tr::scale(p.alpha64, p.alphaIm, acc);
    if (p.beta64 != 0.0 || (Tr::CX && p.betaIm != 0.0))
        val = Tr::apply(W_OP_ADD, val, Tr::scale(p.beta64, p.betaIm, w_un<Tr, UN>(p.unC, Tr::load1(static_cast<const Elem*>(p.C) + rd_offset<2>(p.kept, k), Tr::CX && p.conjC != 0))));
    Tr::store1(static_cast<Elem*>(p.D) + rd_offset<1>(p.kept, k), val);
}

// ---------------------------------------------------------------------------------------------
// RED_GENERIC: any dtype / strides.  One lane per (kept element, split).
// ---------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ double rg_load(const T* p) { return (double)(*p); }
template <> __device__ __forceinline__ double rg_load<__half>(const __half* p) { return (double)__half2float(*p); }
template <> __device__ __forceinline__ double rg_load<__hip_bfloat16>(const __hip_bfloat16* p) { return (double)__bfloat162float(*p); }
template <typename T> __device__ __forceinline__ void rg_store(T* p, double v) { *p = (T)v; }
template <> __device__ __forceinline__ void rg_store<__half>(__half* p, double v) { *p = __float2half((float)v); }
template <> __device__ __forceinline__ void rg_store<__hip_bfloat16>(__hip_bfloat16* p, double v) { *p = __float2bfloat16((float)v); }

// ---------------------------------------------------------------------------------------------
// Complex reductions (HIP_C_32F / HIP_C_64F; python/einsum.h:326-343,430-441 runs a unary einsum on complex tensors through
// cutensorCreateReduction(OP_ADD) + cutensorReduce; einsum.cu:346-372): RED_GENERIC's structure on (re, im) pairs — one lane per
// (kept element, split), complex alpha / beta, conjugation of A / C, ADD and MUL.  Accumulation in the data's own precision
// (like the real kernels: float for complex64, double for complex128); partials are [splitR][kept] pairs.
// ---------------------------------------------------------------------------------------------
template <typename R> struct RdCx { R re, im; };
template <typename R> __device__ __forceinline__ RdCx<R> rc_mul(RdCx<R> a, RdCx<R> b) { return RdCx<R>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename R> __device__ __forceinline__ RdCx<R> rc_apply(int op, RdCx<R> a, RdCx<R> b) {
    return op == OP_MUL ? rc_mul(a, b) : RdCx<R>{a.re + b.re, a.im + b.im};
}
template <typename R> __device__ __forceinline__ void rc_finish(const ReduceParams& p, uint32_t k, RdCx<R> acc) {
    const RdCx<R> alpha = {(R)p.alpha64, (R)p.alphaIm}, beta = {(R)p.beta64, (R)p.betaIm};
    RdCx<R> val = rc_mul(alpha, acc);
    if (beta.re != (R)0 || beta.im != (R)0) {
        RdCx<R> c = static_cast<const RdCx<R>*>(p.C)[rd_offset<2>(p.kept, k)];
        if (p.conjC) c.im = -c.im;
        const RdCx<R> bc = rc_mul(beta, c);
        val.re += bc.re; val.im += bc.im;
    }
    static_cast<RdCx<R>*>(p.D)[rd_offset<1>(p.kept, k)] = val;
}

template <typename R>
__global__ void __launch_bounds__(256) reduce_generic_cplx_kernel(const ReduceParams p) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= p.kept.total) return;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * p.redPerSplit;
    uint32_t rEnd = rBegin + p.redPerSplit;
    if (rEnd > p.red.total) rEnd = p.red.total;
    const int op = p.op;
    const RdCx<R>* A = static_cast<const RdCx<R>*>(p.A) + rd_offset<0>(p.kept, k);
    RdCx<R> acc = {op == OP_MUL ? (R)1 : (R)0, (R)0};
    const R sgn = p.conjA ? (R)-1 : (R)1;
    uint32_t r = rBegin;
    for (; r + 4 <= rEnd; r += 4) {               // four loads in flight (reduce_generic_kernel, round 6); same order of the combines
        RdCx<R> x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = A[rd_offset<0>(p.red, r + (uint32_t)u)];
#pragma unroll
        for (int u = 0; u < 4; ++u) { x[u].im *= sgn; acc = rc_apply<R>(op, acc, x[u]); }
    }
    for (; r < rEnd; ++r) {
        RdCx<R> x = A[rd_offset<0>(p.red, r)];
        x.im *= sgn;
        acc = rc_apply<R>(op, acc, x);
    }
    if (p.partial != nullptr) {
        static_cast<RdCx<R>*>(p.partial)[(size_t)split * p.kept.total + k] = acc;
        return;
    }
    rc_finish<R>(p, k, acc);
}

template <typename R>
__global__ void __launch_bounds__(256) reduce_finalize_cplx_kernel(const ReduceParams p) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= p.kept.total) return;
    const int op = p.op;
    const RdCx<R>* P = static_cast<const RdCx<R>*>(p.partial) + k;
    RdCx<R> acc = {op == OP_MUL ? (R)1 : (R)0, (R)0};
    for (uint32_t s = 0; s < p.splitR; ++s) acc = rc_apply<R>(op, acc, P[(size_t)s * p.kept.total]);
    rc_finish<R>(p, k, acc);
}

// ---------------------------------------------------------------------------------------------
// The kernels of real data, twice (reduce_kernels.inc): x_kernel with UN = false — the identity twins, what ran before the unary
// operators existed, under the same symbols — and x_un_kernel with UN = true, the operator twins (unary_op.h).
// ---------------------------------------------------------------------------------------------
// (the operator twins come first: with them behind the identity twins the compiler laid out reduce_row_f32_kernel's loops differently
// from the build before the operators existed; in this order every identity kernel's machine code is what it was)
#define CTAMD_UN true
#define CTAMD_KERNEL(x) x##_un_kernel
#include "reduce_kernels.inc"
#undef CTAMD_UN
#undef CTAMD_KERNEL
#define CTAMD_UN false
#define CTAMD_KERNEL(x) x##_kernel
#include "reduce_kernels.inc"
#undef CTAMD_UN
#undef CTAMD_KERNEL

// launches the identity twin ID or, when an operand this launch reads carries a unary operator (un), the operator twin UNK
#define CTAMD_RED_TWIN(un, grid, ID, UNK)                                              \
    do {                                                                               \
        if (un) hipLaunchKernelGGL(UNK, grid, dim3(256), 0, stream, p);                \
        else    hipLaunchKernelGGL(ID, grid, dim3(256), 0, stream, p);                 \
    } while (0)

template <class Tr>
static hipError_t launch_wide_t(const ReduceParams& p, int variant, bool un, hipStream_t stream) {
    const dim3 grid = variant == RED_COL ? dim3(((p.kept.total / (uint32_t)Tr::NV) + 255u) / 256u, p.splitR) : dim3((p.kept.total + 3u) / 4u, p.splitR);
    if constexpr (Tr::CX) {
        if (un) return hipErrorInvalidValue;                 // (the planner admits unary operators on real data only)
        if (variant == RED_COL) hipLaunchKernelGGL(reduce_col_wide_kernel<Tr>, grid, dim3(256), 0, stream, p);
        else                    hipLaunchKernelGGL(reduce_row_wide_kernel<Tr>, grid, dim3(256), 0, stream, p);
    } else {
        if (variant == RED_COL) CTAMD_RED_TWIN(un, grid, reduce_col_wide_kernel<Tr>, reduce_col_wide_un_kernel<Tr>);
        else                    CTAMD_RED_TWIN(un, grid, reduce_row_wide_kernel<Tr>, reduce_row_wide_un_kernel<Tr>);
    }
    return hipSuccess;
}

template <typename T, typename S>
static void launch_generic_t(const ReduceParams& p, bool un, hipStream_t stream) {
    if (p.rowAny != 0u) {                         // A's stride-1 mode is reduced: a wave per kept element (reduce_row_any_kernel)
        const dim3 grid((p.kept.total + 3u) / 4u, p.splitR);
        CTAMD_RED_TWIN(un, grid, (reduce_row_any_kernel<T, S>), (reduce_row_any_un_kernel<T, S>));
        return;
    }
    const dim3 grid((p.kept.total + 255u) / 256u, p.splitR);
    CTAMD_RED_TWIN(un, grid, (reduce_generic_kernel<T, S>), (reduce_generic_un_kernel<T, S>));
}
template <typename T, typename S>
static void launch_finalize_t(const ReduceParams& p, bool un, hipStream_t stream) {
    const dim3 grid((p.kept.total + 255u) / 256u);
    CTAMD_RED_TWIN(un, grid, (reduce_finalize_kernel<T, S>), (reduce_finalize_un_kernel<T, S>));
}

hipError_t launch_reduce(const ReduceParams& p, int variant, int dtype, bool acc64, hipStream_t stream) {
    if (p.kept.total == 0) return hipSuccess;
    // the operator twin: A carries a unary operator, or C does and this launch is the one that reads C (no split, beta != 0)
    const bool readsC = p.partial == nullptr && (p.beta64 != 0.0 || p.betaIm != 0.0);
    const bool un = un_active(p.unA) || (readsC && un_active(p.unC));
    if (un && (dtype == HIP_C_32F || dtype == HIP_C_64F)) return hipErrorInvalidValue;
    if (variant == RED_COL && dtype == HIP_R_32F) {
        const dim3 grid(((p.kept.total / 4u) + 255u) / 256u, p.splitR);
        CTAMD_RED_TWIN(un, grid, reduce_col_f32_kernel, reduce_col_f32_un_kernel);
    } else if (variant == RED_ROW && dtype == HIP_R_32F) {
        const dim3 grid((p.kept.total + 3u) / 4u, p.splitR);
        CTAMD_RED_TWIN(un, grid, reduce_row_f32_kernel, reduce_row_f32_un_kernel);
    } else if ((variant == RED_COL || variant == RED_ROW) && dtype != HIP_R_32F && (!acc64 || dtype == HIP_R_64F || dtype == HIP_C_64F)) {
        hipError_t e = hipSuccess;
        switch (dtype) {       // the tiled kernels of the other element types (wide_elem.h)
            case HIP_R_64F:  e = launch_wide_t<WF64>(p, variant, un, stream); break;
            case HIP_R_16F:  e = launch_wide_t<WH16<false>>(p, variant, un, stream); break;
            case HIP_R_16BF: e = launch_wide_t<WH16<true>>(p, variant, un, stream); break;
            case HIP_C_32F:  e = launch_wide_t<WCplx<float>>(p, variant, un, stream); break;
            case HIP_C_64F:  e = launch_wide_t<WCplx<double>>(p, variant, un, stream); break;
            default: return hipErrorInvalidValue;
        }
        if (e != hipSuccess) return e;
    } else if (variant == RED_GENERIC) {
        switch (dtype) {
            case HIP_R_32F:  if (acc64) launch_generic_t<float, double>(p, un, stream); else launch_generic_t<float, float>(p, un, stream); break;
            case HIP_R_64F:  launch_generic_t<double, double>(p, un, stream); break;
            case HIP_R_16F:  launch_generic_t<__half, float>(p, un, stream); break;
            case HIP_R_16BF: launch_generic_t<__hip_bfloat16, float>(p, un, stream); break;
            case HIP_C_32F:  hipLaunchKernelGGL(reduce_generic_cplx_kernel<float>, dim3((p.kept.total + 255u) / 256u, p.splitR), dim3(256), 0, stream, p); break;
            case HIP_C_64F:  hipLaunchKernelGGL(reduce_generic_cplx_kernel<double>, dim3((p.kept.total + 255u) / 256u, p.splitR), dim3(256), 0, stream, p); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_reduce_finalize(const ReduceParams& p, int dtype, bool acc64, hipStream_t stream) {
    if (p.kept.total == 0) return hipSuccess;
    const bool un = un_active(p.unC) && (p.beta64 != 0.0 || p.betaIm != 0.0);     // (unA went into the partials)
    if (un && (dtype == HIP_C_32F || dtype == HIP_C_64F)) return hipErrorInvalidValue;
    switch (dtype) {
        case HIP_R_32F:  if (acc64) launch_finalize_t<float, double>(p, un, stream); else launch_finalize_t<float, float>(p, un, stream); break;
        case HIP_R_64F:  launch_finalize_t<double, double>(p, un, stream); break;
        case HIP_R_16F:  launch_finalize_t<__half, float>(p, un, stream); break;
        case HIP_R_16BF: launch_finalize_t<__hip_bfloat16, float>(p, un, stream); break;
        case HIP_C_32F:  hipLaunchKernelGGL(reduce_finalize_cplx_kernel<float>, dim3((p.kept.total + 255u) / 256u), dim3(256), 0, stream, p); break;
        case HIP_C_64F:  hipLaunchKernelGGL(reduce_finalize_cplx_kernel<double>, dim3((p.kept.total + 255u) / 256u), dim3(256), 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ctamd
