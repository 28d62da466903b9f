// gett_gen_common.h — what the four element paths of the general MFMA GETT family (gett_gen.inc, gett_gen_f32x.inc, gett_gen_f64x.inc,
// gett_gen_c32x.inc) share WITHOUT a change to their compiled kernels: the vector typedefs, the 16-bit MFMA call, the conversion of an fp32
// value to the 16-bit pattern(s) of a reduced-precision mode, the launch wrapper and the kernel-table entry macros.  Device code; the index
// arithmetic of the LDS image is gett_gen_layout.h (plain C++, replayed on the CPU by tests/harness/).
//
// The kernel bodies — tile decode, row and k clamps, the two-stage K loop, the split-K and epilogue walks — are still written out in each
// of the four files.  Moved into __forceinline__ helpers (a tile struct, an operand base class, walks that take the element code as a
// callable) they compile to other code: the kernels keep all of GettParams in scalar registers and spill about 80 of them to vector lanes,
// and every such move shifts which are reloaded where — 2 to 8 % more instructions, a private segment in single 64 x 64 instantiations,
// and 1 to 9 % more time on some 4096^3 shapes.  Everything in this header leaves the disassembly of all kernels as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "params.h"
#include "launch.h"
#include "gett_common.h"
#include "gett_gen_layout.h"

namespace ctamd {

typedef double   f64x4 __attribute__((ext_vector_type(4)));
typedef double   f64x2 __attribute__((ext_vector_type(2)));
typedef float    f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short    g16x8 __attribute__((ext_vector_type(8)));
typedef __bf16   gbf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 gf16x8 __attribute__((ext_vector_type(8)));

// one v_mfma_f32_16x16x32_{f16,bf16} on two 16-byte fragments of 16-bit patterns
template <bool F16>
__device__ __forceinline__ f32x4 gen_mfma16(const g16x8& a, const g16x8& b, f32x4 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gf16x8, a), __builtin_bit_cast(gf16x8, b), c, 0, 0, 0);
    else               return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gbf16x8, a), __builtin_bit_cast(gbf16x8, b), c, 0, 0, 0);
}

// fp32 -> the 16-bit pattern(s) of a reduced-precision mode (gett_gen_f32x.inc: an element; gett_gen_c32x.inc: each part of one).
// PLANES = 2: (hi, lo) of the three-term split; a value whose bf16 rounding is not finite goes to the lo plane whole, with hi = 0.
enum Gen16Mode : int { GEN16_BF16 = 0, GEN16_F16 = 1, GEN16_BF16X3 = 2 };      // the order of GEN_F32_* and of GEN_C32_* in GenElem
template <int MODE> struct Gen16Cvt {
    static constexpr int PLANES = 1;
    static __device__ __forceinline__ void cvt(float x, uint16_t (&o)[1]) {
        if constexpr (MODE == GEN16_F16) o[0] = __builtin_bit_cast(uint16_t, (_Float16)x);
        else                             o[0] = __builtin_bit_cast(uint16_t, (__bf16)x);
    }
};
template <> struct Gen16Cvt<GEN16_BF16X3> {
    static constexpr int PLANES = 2;
    static __device__ __forceinline__ void cvt(float x, uint16_t (&o)[2]) {
        const __bf16 hi = (__bf16)x;
        const uint16_t hb = __builtin_bit_cast(uint16_t, hi);
        const bool finite = (hb & 0x7f80u) != 0x7f80u;
        const float rest = finite ? x - (float)hi : x;      // exact; a non-finite value goes to the lo plane whole
        o[0] = finite ? hb : (uint16_t)0;
        o[1] = __builtin_bit_cast(uint16_t, (__bf16)rest);
    }
};

template <void (*KERNEL)(const GettParams)>
static hipError_t launch_gen_family(const GettParams& p, hipStream_t stream) {
    if (p.nBlocks == 0) return hipSuccess;
    hipLaunchKernelGGL(KERNEL, dim3(p.nBlocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// table entry: {bm, bn, bk, wm, wn, wk, layA, layB, threads, pf, kfast, ablation, launch, fragPartials, nt, elem, vec, name}
#define CTAMD_GEN_FAMILY_ENTRY(KERNEL, CFG, GE, BM, BN, BK, OA, OB, V) \
    {BM, BN, BK, 2, 2, 1, OA, OB, 256, 1, 0, 0, &launch_gen_family<KERNEL<CFG<GE, BM, BN, BK, OA, OB, V>>>, 0, 0, GE, V, #KERNEL},
// the four orientation pairs (LAY_F = 0: free-contiguous, LAY_K = 1: K-contiguous) of one (element, tile, vector width)
#define CTAMD_GEN_FAMILY_ORIENTS(KERNEL, CFG, GE, BM, BN, BK, V)   \
    CTAMD_GEN_FAMILY_ENTRY(KERNEL, CFG, GE, BM, BN, BK, 0, 0, V)   \
    CTAMD_GEN_FAMILY_ENTRY(KERNEL, CFG, GE, BM, BN, BK, 0, 1, V)   \
    CTAMD_GEN_FAMILY_ENTRY(KERNEL, CFG, GE, BM, BN, BK, 1, 0, V)   \
    CTAMD_GEN_FAMILY_ENTRY(KERNEL, CFG, GE, BM, BN, BK, 1, 1, V)

}  // namespace ctamd
