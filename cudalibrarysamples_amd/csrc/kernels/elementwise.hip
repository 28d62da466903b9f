// elementwise.hip — HBM-bound strided copy / permutation kernels for gfx950.
//
// Replaces the closed kernels behind cutensorPermute (reference call site:
// cuTENSOR/elementwise_permute.cu:198-200, "C_{c,w,h,n} = alpha * A_{w,h,c,n}" :51-63),
// cutensorElementwiseBinaryExecute (cuTENSOR/elementwise_binary.cu:202-205) and the permutation-only
// use of cutensorReduce by the einsum helper (cuTENSOR/einsum.cu:449-450).
//
// Every tensor is walked through strides; nothing is reshaped.  The planner hands over two tile
// modes plus a linearised remainder (Ew2DParams).  Roofline: HBM; algorithmic bytes per element =
// 2 * sizeof(T) (+ sizeof(T) when a gamma*C term is read) — elementwise_permute.cu:208.
//
//   EW_TRANSPOSE  D's stride-1 mode (dim0) differs from A's stride-1 mode (dim1).  A T0 x 64 tile (T0 = 64 / 128 / 256
//                 along dim0, chosen by the planner: the width of the WRITTEN row segment is what decides the rate) is read
//                 with 16-byte lanes along dim1 (256-B contiguous segments per row), transposed 4x4 in registers, parked in
//                 LDS as [dim1][dim0] and written with 16-byte lanes along dim0 (256-B / 512-B / 1-KiB segments).  One
//                 workgroup per tile; interior tiles take an unguarded path (all loads issued before the first use); for
//                 doubly-strided transposes the tile order goes rest-first with one contiguous eighth per XCD.  16-bit data:
//                 the same with 8 x 8 register transposes on {128, 256} x {64, 128} tiles (ew_transpose_h16_wide_kernel).
//   EW_ROWCOPY    A and D share the stride-1 mode: 16-byte lanes along it, 8 dim1-rows per
//                 workgroup, no LDS.
//   EW_GENERIC    anything else (odd extents, unaligned bases, 2- and 8-byte types): one element
//                 per lane, lanes along dim0.
//
// A and D (and C) have ONE data type here; the kernels that read one element width and write another (cutensorPermute and the binary
// form with an output of another type: ew_rowcopy_convert_kernel, ew_transpose_convert_kernel, ew_generic_convert_kernel) are
// elementwise_convert.hip, and the device helpers both files use are elementwise_common.h.
//
// The kernels of real data are in elementwise_kernels.inc, which this file includes twice: as x_kernel (the identity twins) and as
// x_un_kernel (the twins that apply the operands' unary operators, unary_op.h).  The sections below keep each family's constants and
// device helpers; the launchers at the end pick variant, type and twin.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <cstring>

#include "elementwise_common.h"
#include "launch.h"
#include "params.h"
#include "unary_op.h"
#include "wide_elem.h"

namespace ctamd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 ew_comb4(int op, f32x4 x, f32x4 y) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = ew_comb<float>(op, x[e], y[e]);
    return r;
}

// ---------------------------------------------------------------------------------------------
// EW_TRANSPOSE (fp32): requires sD0 == 1, sA1 == 1, E0 % 4 == 0, E1 % 4 == 0, every other stride
// a multiple of 4 elements and 16-byte aligned bases.
// ---------------------------------------------------------------------------------------------
constexpr int TT = 64;          // tile extent along dim1 (A's contiguous mode: 256-B read segments); also the h16 kernels' edge


// ---------------------------------------------------------------------------------------------
// EW_ROWCOPY (fp32): sD0 == 1 and sA0 == 1, E0 % 4 == 0, other strides multiples of 4, aligned.
// Tile = 256 dim0 elements (64 lanes x float4) x 8 dim1 rows (4 waves x 2 rows).
// ---------------------------------------------------------------------------------------------
constexpr int RC_T0 = 256, RC_T1 = 8;


// ---------------------------------------------------------------------------------------------
// 16-bit data (bf16 / fp16), same two shapes: 16-byte lanes = 8 elements, arithmetic in fp32.
//   EW_ROWCOPY   tile = 512 dim0 elements (64 lanes x 8) x 8 dim1 rows
//   EW_TRANSPOSE tile = 64 x 64 elements; LDS image [dim1][dim0] with an odd row pitch (65 elements), filled and
//                drained with 2-byte LDS accesses (16 + 16 per lane and tile — a few hundred LDS cycles against
//                ~2 k cycles of HBM time for the tile's 16 KiB), HBM sees 128-byte segments on both sides
// ---------------------------------------------------------------------------------------------
template <bool BF> __device__ __forceinline__ void h16_unpack(u32x4e v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = h16_to_f32<BF>((uint16_t)(v[i] & 0xffffu)); f[2 * i + 1] = h16_to_f32<BF>((uint16_t)(v[i] >> 16)); }
}
template <bool BF> __device__ __forceinline__ u32x4e h16_pack(const float (&f)[8]) {
    u32x4e v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (uint32_t)f32_to_h16<BF>(f[2 * i]) | ((uint32_t)f32_to_h16<BF>(f[2 * i + 1]) << 16);
    return v;
}
// out = opAC(opAB(delta * unE(E), alpha * unA(a)), gamma * unC(C)) on 8 elements starting at D-offset offD (dim0 contiguous)
template <bool BF, bool UN>
__device__ __forceinline__ u32x4e h16_combine(const Ew2DParams& p, const float (&a)[8], const uint16_t* E, const uint16_t* C,
                                              int64_t offD, int64_t offC) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = a[i];
    un_apply_n<UN, float, 8>(p.unA, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p.alpha * v[i];
    if (E != nullptr) {
        float e[8];
        h16_unpack<BF>(*reinterpret_cast<const u32x4e*>(E + offD), e);
        un_apply_n<UN, float, 8>(p.unE, e);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ew_comb<float>(p.opAB, p.delta * e[i], v[i]);
    }
    if (C != nullptr) {
        float c[8];
        if (p.sC0 == 1) {
            h16_unpack<BF>(*reinterpret_cast<const u32x4e*>(C + offC), c);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = h16_to_f32<BF>(C[offC + (int64_t)i * p.sC0]);
        }
        un_apply_n<UN, float, 8>(p.unC, c);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ew_comb<float>(p.opAC, v[i], p.gamma * c[i]);
    }
    return h16_pack<BF>(v);
}

// ---------------------------------------------------------------------------------------------
// EW_GENERIC: any strides / dtype.  Tile = 64 dim0 elements x 4 dim1 rows, one element per lane.
// ---------------------------------------------------------------------------------------------
constexpr int GN_T0 = 64, GN_T1 = 4;

template <typename T> struct EwScalar { typedef float type; };
template <> struct EwScalar<double> { typedef double type; };

template <typename T> __device__ __forceinline__ typename EwScalar<T>::type ew_load(const T* p) { return (typename EwScalar<T>::type)(*p); }
template <> __device__ __forceinline__ float ew_load<__half>(const __half* p) { return __half2float(*p); }
template <> __device__ __forceinline__ float ew_load<__hip_bfloat16>(const __hip_bfloat16* p) { return __bfloat162float(*p); }
template <typename T> __device__ __forceinline__ void ew_store(T* p, typename EwScalar<T>::type v) { *p = (T)v; }
template <> __device__ __forceinline__ void ew_store<__half>(__half* p, float v) { *p = __float2half(v); }
template <> __device__ __forceinline__ void ew_store<__hip_bfloat16>(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }


// ---------------------------------------------------------------------------------------------
// EW_BLOCK (round 6): D = alpha * perm(A) where the leading modes of D are the same packed set as the leading modes of A — every index
// of the other modes owns a block of blkTotal elements that is contiguous in A and in D and only permuted inside.  A workgroup loads
// blkGroup such blocks into LDS as they lie (coalesced), and writes them out in D's order (coalesced) through permuted LDS reads:
// 2 |D| bytes, no strided global access.  What the element-gather kernel above does with such a tensor: 13 MB of bf16 from
// [d = 50, c = 16, b = 4 | a] to [b, c, d | a] in 380 us (each lane of a store reads another 64-byte line); this kernel: one pass at the
// rate of a copy.  alpha == 1 moves the bits untouched.  HBM-bound.
// ---------------------------------------------------------------------------------------------

// VEC: elements per 16-byte lane when the planner found 16-byte lanes on both sides (blkVec: block size, rest strides and base alignment
// multiples of it) — blocks are loaded 16 bytes per lane, and a lane gathers VEC consecutive output elements from LDS for ONE 16-byte
// store; VEC = 1: element by element (any extents / alignment).
template <typename T, int VEC>
__global__ void __launch_bounds__(256) ew_block_kernel(const Ew2DParams p) {
    // (dynamic LDS, sized to the group's blocks: a 6-KiB block leaves room for eight workgroups per CU where a static 32 KiB allowed five)
    extern __shared__ __attribute__((aligned(16))) unsigned char ew_block_lds[];
    T* const lds = reinterpret_cast<T*>(ew_block_lds);
    const T* A = static_cast<const T*>(p.A);
    T*       D = static_cast<T*>(p.D);
    const uint32_t P = p.blkTotal;
    const uint32_t r0 = blockIdx.x * p.blkGroup;
    const uint32_t nG = (p.blkRest.total - r0 < p.blkGroup) ? (p.blkRest.total - r0) : p.blkGroup;
    const int tid = threadIdx.x;
    struct alignas(16) Lane { T v[VEC]; };
    for (uint32_t g = 0; g < nG; ++g) {
        int64_t oA, oD, oC;
        rest_offsets(p.blkRest, r0 + g, oA, oD, oC);
        const T* src = A + oA;
        T* dst = lds + g * P;
        if constexpr (VEC > 1) {
            for (uint32_t e = tid * VEC; e < P; e += 256 * VEC) *reinterpret_cast<Lane*>(dst + e) = *reinterpret_cast<const Lane*>(src + e);
        } else {
            for (uint32_t e = tid; e < P; e += 256) dst[e] = src[e];
        }
    }
    __syncthreads();
    const bool raw = p.alpha == 1.0f;
    auto src_index = [&](uint32_t f) {
        uint32_t rem = f, idx = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < (int)p.blkN) {
                const uint32_t q = (i + 1 < (int)p.blkN) ? ew_fast_div(rem, p.blkDiv[i]) : 0u;
                idx += (rem - q * p.blkDiv[i].d) * p.blkSrc[i];
                rem = q;
            }
        }
        return idx;
    };
    for (uint32_t g = 0; g < nG; ++g) {
        int64_t oA, oD, oC;
        rest_offsets(p.blkRest, r0 + g, oA, oD, oC);
        const T* src = lds + g * P;
        T* dst = D + oD;
        if constexpr (VEC > 1) {
            for (uint32_t f = tid * VEC; f < P; f += 256 * VEC) {
                // the digits of f once (three divisions), then VEC - 1 increments with carry: the lane's VEC consecutive output elements
                uint32_t dig[4], rem = f, idx = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t q = (i + 1 < (int)p.blkN) ? ew_fast_div(rem, p.blkDiv[i]) : 0u;
                    dig[i] = (i < (int)p.blkN) ? rem - q * p.blkDiv[i].d : 0u;
                    idx += dig[i] * p.blkSrc[i];
                    rem = q;
                }
                Lane out;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const T v = src[idx];
                    if (raw) out.v[j] = v;
                    else { T w; ew_store<T>(&w, p.alpha * ew_load<T>(&v)); out.v[j] = w; }
                    if (j + 1 < VEC) {
                        bool carry = true;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            if (carry && i < (int)p.blkN) {
                                dig[i] += 1u; idx += p.blkSrc[i];
                                carry = dig[i] == p.blkDiv[i].d;
                                if (carry) { idx -= dig[i] * p.blkSrc[i]; dig[i] = 0u; }
                            }
                        }
                    }
                }
                *reinterpret_cast<Lane*>(dst + f) = out;
            }
        } else {
            for (uint32_t f = tid; f < P; f += 256) {
                const uint32_t idx = src_index(f);
                if (raw) dst[f] = src[idx];
                else ew_store<T>(dst + f, p.alpha * ew_load<T>(src + idx));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// EW_GENERIC for complex data (HIP_C_32F / HIP_C_64F): what the reference's binding runs for a unary einsum on complex tensors
// (python/einsum.h:326-343,430-441: cutensorCreateReduction + cutensorReduce with no reduced mode = a permutation;
// torch/einsum.cc:83 dispatches the complex types) and cutensorPermute / cutensorElementwiseBinaryExecute on complex tensors.
//   D = opAC(alpha * op(perm(A)), gamma * op(perm(C)))      alpha, gamma complex; op in {IDENTITY, CONJ}; opAC in {ADD, MUL}
// One (re, im) pair per lane: 8- / 16-byte loads and stores, 512 B / 1 KiB per wave along D's fastest mode.  Same tile
// decomposition as ew_generic_kernel (64 dim0 elements x 4 dim1 rows).  HBM-bound: 2 |D| bytes (+ |C|).
// ---------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(256) ew_generic_cplx_kernel(const Ew2DParams p) {
    typedef WCx<R> T;                 // (re, im) pairs and their arithmetic: wide_elem.h
    const T* A = static_cast<const T*>(p.A);
    const T* C = static_cast<const T*>(p.C);
    T*       D = static_cast<T*>(p.D);
    const T alpha = {(R)p.alpha64, (R)p.alphaIm}, gamma = {(R)p.gamma64, (R)p.gammaIm};
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * GN_T0 + (tid & 63);
        const uint32_t r1 = t.t1 * GN_T1 + (tid >> 6);
        if (c0 >= p.E0 || r1 >= p.E1) continue;
        T a = A[oA + (int64_t)c0 * p.sA0 + (int64_t)r1 * p.sA1];
        if (p.conjA) a.im = -a.im;
        T v = wcx_mul(alpha, a);
        if (C != nullptr) {
            T c = C[oC + (int64_t)c0 * p.sC0 + (int64_t)r1 * p.sC1];
            if (p.conjC) c.im = -c.im;
            v = WCplx<R>::apply(p.opAC, v, wcx_mul(gamma, c));     // MUL, else ADD (the planner admits nothing else)
        }
        D[oD + (int64_t)c0 * p.sD0 + (int64_t)r1 * p.sD1] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// EW_TRANSPOSE / EW_ROWCOPY for 8- and 16-byte elements (fp64, complex64, complex128; round 6, wide_elem.h):
//   D = opAC(alpha * op(perm(A)), gamma * op(C))       op in {IDENTITY, CONJ}; opAC: ADD / MUL (+ MAX / MIN on fp64)
// the fp32 kernels' structure with a 16-byte lane = Tr::NV elements (2 / 2 / 1).  Transposing form: a T0 x T1 tile (T0 along dim0 = D's
// stride-1 mode: 1-KiB written row segments; T1 along dim1 = A's stride-1 mode: 256-B read segments) is read with 16-byte lanes along
// dim1, NV rows per lane, transposed NV x NV in registers, parked in LDS as [dim1][dim0] and written with 16-byte lanes along dim0.
// Planner conditions (plan_elementwise): sD0 == 1, sA1 == 1 (transposing) or sA0 == 1 (row copy), extents and every other stride
// multiples of NV, 16-byte-aligned descriptors, no E / X operand.  HBM-bound: 2 |D| bytes (+ |C|).
// ---------------------------------------------------------------------------------------------
template <class Tr, bool UN>
__device__ __forceinline__ typename Tr::Acc w_ew_finish(const Ew2DParams& p, typename Tr::Acc a, const typename Tr::Elem* cp, bool hasC) {
    typename Tr::Acc v = Tr::scale(p.alpha64, p.alphaIm, w_un<Tr, UN>(p.unA, a));
    if (hasC) v = Tr::apply(p.opAC == 0 ? W_OP_ADD : p.opAC, v, Tr::scale(p.gamma64, p.gammaIm, w_un<Tr, UN>(p.unC, Tr::load1(cp, Tr::CX && p.conjC != 0))));
    return v;
}

// ---------------------------------------------------------------------------------------------
// The kernels, twice (elementwise_kernels.inc): x_kernel with UN = false — the identity twins, what ran before the unary operators
// existed, under the same symbols — and x_un_kernel with UN = true, the operator twins (unary_op.h).
// ---------------------------------------------------------------------------------------------
#define CTAMD_UN false
#define CTAMD_KERNEL(x) x##_kernel
#include "elementwise_kernels.inc"
#undef CTAMD_UN
#undef CTAMD_KERNEL
#define CTAMD_UN true
#define CTAMD_KERNEL(x) x##_un_kernel
#include "elementwise_kernels.inc"
#undef CTAMD_UN
#undef CTAMD_KERNEL

// launches the identity twin ID or, when an attached operand carries a unary operator (un), the operator twin UNK
#define CTAMD_EW_TWIN(un, grid, ID, UNK)                                                      \
    do {                                                                                      \
        if (un) hipLaunchKernelGGL(UNK, dim3(grid), dim3(256), 0, stream, p);                 \
        else    hipLaunchKernelGGL(ID, dim3(grid), dim3(256), 0, stream, p);                  \
    } while (0)

template <bool BF>
static void launch_h16_wide(const Ew2DParams& p, bool un, unsigned grid, hipStream_t stream) {
    if (p.tile0 == 256 && p.tile1 == 128)      CTAMD_EW_TWIN(un, grid, (ew_transpose_h16_wide_kernel<BF, 256, 128>), (ew_transpose_h16_wide_un_kernel<BF, 256, 128>));
    else if (p.tile0 == 256)                   CTAMD_EW_TWIN(un, grid, (ew_transpose_h16_wide_kernel<BF, 256, 64>), (ew_transpose_h16_wide_un_kernel<BF, 256, 64>));
    else if (p.tile1 == 128)                   CTAMD_EW_TWIN(un, grid, (ew_transpose_h16_wide_kernel<BF, 128, 128>), (ew_transpose_h16_wide_un_kernel<BF, 128, 128>));
    else                                       CTAMD_EW_TWIN(un, grid, (ew_transpose_h16_wide_kernel<BF, 128, 64>), (ew_transpose_h16_wide_un_kernel<BF, 128, 64>));
}

template <class Tr, int T0, int T1>
static hipError_t launch_wide_ew(const Ew2DParams& p, int variant, bool un, unsigned grid, hipStream_t stream) {
    if (p.E != nullptr || p.X != nullptr) return hipErrorInvalidValue;    // the planner never pairs these variants with a trinary operand
    if constexpr (Tr::CX) {
        if (un) return hipErrorInvalidValue;                              // (the planner admits unary operators on real data only)
        if (variant == EW_TRANSPOSE) hipLaunchKernelGGL((ew_transpose_wide_kernel<Tr, T0, T1>), dim3(grid), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(ew_rowcopy_wide_kernel<Tr>, dim3(grid), dim3(256), 0, stream, p);
    } else {
        if (variant == EW_TRANSPOSE) CTAMD_EW_TWIN(un, grid, (ew_transpose_wide_kernel<Tr, T0, T1>), (ew_transpose_wide_un_kernel<Tr, T0, T1>));
        else CTAMD_EW_TWIN(un, grid, ew_rowcopy_wide_kernel<Tr>, ew_rowcopy_wide_un_kernel<Tr>);
    }
    return hipGetLastError();
}

// Contiguous fill with 16-byte stores (HBM-bound: n * sizeof(T) bytes written).  The base needs the element's alignment only: the bytes
// up to the first 16-byte boundary (head) and those behind the last whole lane (tail) are written one per thread.  The pattern's period
// is the element size, which divides 16 and the head's length, so head, body and tail all index it from byte 0.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct FillPattern { uint32_t w[4]; };

__global__ void __launch_bounds__(256) ew_fill_kernel(u32x4* D16, uint64_t n16, unsigned char* head, uint32_t headBytes, unsigned char* tail,
                                                      uint32_t tailBytes, FillPattern pat) {
    const u32x4 v = {pat.w[0], pat.w[1], pat.w[2], pat.w[3]};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride)
        __builtin_nontemporal_store(v, D16 + i);
    if (blockIdx.x == 0) {
        const unsigned char b = (unsigned char)(pat.w[(threadIdx.x >> 2) & 3] >> (8 * (threadIdx.x & 3)));
        if (threadIdx.x < headBytes) head[threadIdx.x] = b;
        if (threadIdx.x < tailBytes) tail[threadIdx.x] = b;
    }
}

static uint16_t fill_f32_to_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static uint16_t fill_f32_to_f16(float f) {   // round to nearest even, host-side
    const _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

hipError_t launch_fill(void* D, uint64_t n, int dtype, double value, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    FillPattern pat;
    size_t es;
    switch (dtype) {
        case HIP_R_32F: { const float v = (float)value; uint32_t u; std::memcpy(&u, &v, 4); pat = FillPattern{{u, u, u, u}}; es = 4; break; }
        case HIP_R_64F: { uint64_t u; std::memcpy(&u, &value, 8); pat = FillPattern{{(uint32_t)u, (uint32_t)(u >> 32), (uint32_t)u, (uint32_t)(u >> 32)}}; es = 8; break; }
        case HIP_R_16F: { const uint32_t u = fill_f32_to_f16((float)value), w = u | (u << 16); pat = FillPattern{{w, w, w, w}}; es = 2; break; }
        case HIP_R_16BF: { const uint32_t u = fill_f32_to_bf16((float)value), w = u | (u << 16); pat = FillPattern{{w, w, w, w}}; es = 2; break; }
        // complex: the padding value is real (CUTENSOR_OPERATION_DESCRIPTOR_PADDING_VALUE is read as one scalar), imaginary part 0
        case HIP_C_32F: { const float v = (float)value; uint32_t u; std::memcpy(&u, &v, 4); pat = FillPattern{{u, 0u, u, 0u}}; es = 8; break; }
        case HIP_C_64F: { uint64_t u; std::memcpy(&u, &value, 8); pat = FillPattern{{(uint32_t)u, (uint32_t)(u >> 32), 0u, 0u}}; es = 16; break; }
        default: return hipErrorInvalidValue;
    }
    const uintptr_t base = reinterpret_cast<uintptr_t>(D);
    if (base % es != 0) return hipErrorInvalidValue;   // (a padded permutation's output, a block of a block-sparse D: the element's alignment)
    const uint64_t bytes = n * es;
    const uint32_t headBytes = (uint32_t)std::min<uint64_t>(bytes, (16 - (base & 15)) & 15);
    const uint64_t n16 = (bytes - headBytes) / 16;
    const uint32_t tailBytes = (uint32_t)((bytes - headBytes) % 16);
    uint64_t blocks = (n16 + 255) / 256;
    if (blocks > 256u * 32u) blocks = 256u * 32u;
    if (blocks == 0) blocks = 1;
    unsigned char* body = static_cast<unsigned char*>(D) + headBytes;
    hipLaunchKernelGGL(ew_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<u32x4*>(body), n16,
                       static_cast<unsigned char*>(D), headBytes, body + n16 * 16, tailBytes, pat);
    return hipGetLastError();
}

hipError_t launch_elementwise(const Ew2DParams& p, int variant, int dtype, hipStream_t stream) {
    if (p.nBlocks == 0) return hipSuccess;
    // the operator twin of a kernel runs when an operand that this launch reads carries a unary operator (unary_op.h); every other
    // launch runs the kernel it always ran
    const bool un = un_active(p.unA) || (p.X != nullptr && un_active(p.unX)) || (p.E != nullptr && un_active(p.unE)) ||
                    (p.C != nullptr && un_active(p.unC));
    if (un && (dtype == HIP_C_32F || dtype == HIP_C_64F)) return hipErrorInvalidValue;
    if (variant == EW_BLOCK) {
        // (the plan keeps the element-gather kernel's decomposition beside the block form: an attached C / E / X operand or a unary
        // operator falls back to it)
        if (!un && p.blkN >= 2 && p.C == nullptr && p.E == nullptr && p.X == nullptr && p.blkBlocks > 0) {
            const bool vec = p.blkVec != 0u && (reinterpret_cast<uintptr_t>(p.A) & 15u) == 0u && (reinterpret_cast<uintptr_t>(p.D) & 15u) == 0u;
            const size_t esz = dtype == HIP_R_32F ? 4 : 2;
            const unsigned ldsBytes = (unsigned)(((size_t)p.blkTotal * p.blkGroup * esz + 15) & ~(size_t)15);
            switch (dtype) {
                case HIP_R_32F:
                    if (vec) hipLaunchKernelGGL((ew_block_kernel<float, 4>), dim3(p.blkBlocks), dim3(256), ldsBytes, stream, p);
                    else     hipLaunchKernelGGL((ew_block_kernel<float, 1>), dim3(p.blkBlocks), dim3(256), ldsBytes, stream, p);
                    return hipGetLastError();
                case HIP_R_16F:
                    if (vec) hipLaunchKernelGGL((ew_block_kernel<__half, 8>), dim3(p.blkBlocks), dim3(256), ldsBytes, stream, p);
                    else     hipLaunchKernelGGL((ew_block_kernel<__half, 1>), dim3(p.blkBlocks), dim3(256), ldsBytes, stream, p);
                    return hipGetLastError();
                case HIP_R_16BF:
                    if (vec) hipLaunchKernelGGL((ew_block_kernel<__hip_bfloat16, 8>), dim3(p.blkBlocks), dim3(256), ldsBytes, stream, p);
                    else     hipLaunchKernelGGL((ew_block_kernel<__hip_bfloat16, 1>), dim3(p.blkBlocks), dim3(256), ldsBytes, stream, p);
                    return hipGetLastError();
                default: break;
            }
        }
        variant = EW_GENERIC;
    }
    const unsigned grid = ew_tiled_grid(p, variant);
    if (variant == EW_TRANSPOSE_ANY) {
        if (p.E != nullptr || p.X != nullptr) return hipErrorInvalidValue;   // (planned for permutations and the binary form only)
        if (p.C != nullptr) {
            switch (dtype) {
                case HIP_R_32F:  CTAMD_EW_TWIN(un, grid, (ew_transpose_any_kernel<float, true>), (ew_transpose_any_un_kernel<float, true>)); return hipGetLastError();
                case HIP_R_16F:  CTAMD_EW_TWIN(un, grid, (ew_transpose_any_kernel<__half, true>), (ew_transpose_any_un_kernel<__half, true>)); return hipGetLastError();
                case HIP_R_16BF: CTAMD_EW_TWIN(un, grid, (ew_transpose_any_kernel<__hip_bfloat16, true>), (ew_transpose_any_un_kernel<__hip_bfloat16, true>)); return hipGetLastError();
                default: return hipErrorInvalidValue;
            }
        }
        if (p.tile0 == 128u && (dtype == HIP_R_16F || dtype == HIP_R_16BF)) {     // the pair form (planned for even extents / strides)
            if (((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.D)) & 3u) != 0u) return hipErrorInvalidValue;
            if (dtype == HIP_R_16F) CTAMD_EW_TWIN(un, grid, ew_transpose_any_pair_kernel<__half>, ew_transpose_any_pair_un_kernel<__half>);
            else                    CTAMD_EW_TWIN(un, grid, ew_transpose_any_pair_kernel<__hip_bfloat16>, ew_transpose_any_pair_un_kernel<__hip_bfloat16>);
            return hipGetLastError();
        }
        switch (dtype) {
            case HIP_R_32F:  CTAMD_EW_TWIN(un, grid, (ew_transpose_any_kernel<float, false>), (ew_transpose_any_un_kernel<float, false>)); return hipGetLastError();
            case HIP_R_16F:  CTAMD_EW_TWIN(un, grid, (ew_transpose_any_kernel<__half, false>), (ew_transpose_any_un_kernel<__half, false>)); return hipGetLastError();
            case HIP_R_16BF: CTAMD_EW_TWIN(un, grid, (ew_transpose_any_kernel<__hip_bfloat16, false>), (ew_transpose_any_un_kernel<__hip_bfloat16, false>)); return hipGetLastError();
            default: return hipErrorInvalidValue;
        }
    }
    if (variant == EW_TRANSPOSE && dtype == HIP_R_32F) {
        if (p.X != nullptr) {
            if (p.tile0 == 128) CTAMD_EW_TWIN(un, grid, (ew_transpose_f32_kernel<true, 128>), (ew_transpose_f32_un_kernel<true, 128>));
            else                CTAMD_EW_TWIN(un, grid, (ew_transpose_f32_kernel<true, 64>), (ew_transpose_f32_un_kernel<true, 64>));
        } else {
            if (p.tile0 == 256)      CTAMD_EW_TWIN(un, grid, (ew_transpose_f32_kernel<false, 256>), (ew_transpose_f32_un_kernel<false, 256>));
            else if (p.tile0 == 128) CTAMD_EW_TWIN(un, grid, (ew_transpose_f32_kernel<false, 128>), (ew_transpose_f32_un_kernel<false, 128>));
            else                     CTAMD_EW_TWIN(un, grid, (ew_transpose_f32_kernel<false, 64>), (ew_transpose_f32_un_kernel<false, 64>));
        }
    } else if (variant == EW_ROWCOPY && dtype == HIP_R_32F) {
        CTAMD_EW_TWIN(un, grid, ew_rowcopy_f32_kernel, ew_rowcopy_f32_un_kernel);
    } else if (variant == EW_TRANSPOSE && (dtype == HIP_R_16BF || dtype == HIP_R_16F)) {
        const bool bf = dtype == HIP_R_16BF;
        if (p.tile0 > 64) {
            if (bf) launch_h16_wide<true>(p, un, grid, stream); else launch_h16_wide<false>(p, un, grid, stream);
        } else {
            if (bf) CTAMD_EW_TWIN(un, grid, ew_transpose_h16_kernel<true>, ew_transpose_h16_un_kernel<true>);
            else    CTAMD_EW_TWIN(un, grid, ew_transpose_h16_kernel<false>, ew_transpose_h16_un_kernel<false>);
        }
    } else if (variant == EW_ROWCOPY && dtype == HIP_R_16BF) {
        CTAMD_EW_TWIN(un, grid, ew_rowcopy_h16_kernel<true>, ew_rowcopy_h16_un_kernel<true>);
    } else if (variant == EW_ROWCOPY && dtype == HIP_R_16F) {
        CTAMD_EW_TWIN(un, grid, ew_rowcopy_h16_kernel<false>, ew_rowcopy_h16_un_kernel<false>);
    } else if ((variant == EW_TRANSPOSE || variant == EW_ROWCOPY) && dtype == HIP_R_64F) {
        return launch_wide_ew<WF64, 128, 32>(p, variant, un, grid, stream);
    } else if ((variant == EW_TRANSPOSE || variant == EW_ROWCOPY) && dtype == HIP_C_32F) {
        return launch_wide_ew<WCplx<float>, 128, 32>(p, variant, un, grid, stream);
    } else if ((variant == EW_TRANSPOSE || variant == EW_ROWCOPY) && dtype == HIP_C_64F) {
        return launch_wide_ew<WCplx<double>, 64, 32>(p, variant, un, grid, stream);
    } else if (variant == EW_GENERIC) {
        switch (dtype) {
            case HIP_R_32F:  CTAMD_EW_TWIN(un, grid, ew_generic_kernel<float>, ew_generic_un_kernel<float>); break;
            case HIP_R_64F:  CTAMD_EW_TWIN(un, grid, ew_generic_kernel<double>, ew_generic_un_kernel<double>); break;
            case HIP_R_16F:  CTAMD_EW_TWIN(un, grid, ew_generic_kernel<__half>, ew_generic_un_kernel<__half>); break;
            case HIP_R_16BF: CTAMD_EW_TWIN(un, grid, ew_generic_kernel<__hip_bfloat16>, ew_generic_un_kernel<__hip_bfloat16>); break;
            case HIP_C_32F:  if (p.E != nullptr || p.X != nullptr) return hipErrorInvalidValue;
                             hipLaunchKernelGGL(ew_generic_cplx_kernel<float>, dim3(grid), dim3(256), 0, stream, p); break;
            case HIP_C_64F:  if (p.E != nullptr || p.X != nullptr) return hipErrorInvalidValue;
                             hipLaunchKernelGGL(ew_generic_cplx_kernel<double>, dim3(grid), dim3(256), 0, stream, p); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ctamd
