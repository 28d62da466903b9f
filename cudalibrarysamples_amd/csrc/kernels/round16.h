// round16.h — the final rounding of every contraction kernel that stores bf16 or fp16: D = rnd16(v + beta * c), v = alpha * acc in fp32.
//
// The contract (tests/test_gpu_round16_exact.py compares it bit for bit):
//   bf16: an fp32 fused multiply-add, then ONE conversion to nearest even — rnd16(rnd32(v + beta * c)).
//   fp16: the fused multiply-add rounded ONCE, straight to 16 bits (v_fma_mixlo_f16) — rnd16(v + beta * c).
// Written as `v += beta * (float)c; (_Float16)v` the compiler picks per call site between v_fma_mixlo_f16 and v_fma_mix_f32 +
// v_cvt_f16_f32 (an fp32 sum rounded a second time), depending on how the neighbours vectorise: kernels of one plan family then differ
// in the last bit where beta * c lies below fp32's last place.  Every epilogue that adds beta * C to a 16-bit result goes through here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ctamd {

template <bool BF>
__device__ __forceinline__ uint16_t h_round16(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (BF) return __builtin_bit_cast(uint16_t, (__bf16)f);      // round to nearest even, NaN stays NaN
    else              return __builtin_bit_cast(uint16_t, (_Float16)f);
#else
    (void)f; return 0;
#endif
}

// round16(v + beta * c), c a 16-bit value of the tensor's type, with ONE rounding.  bf16: the fma is an fp32 operation whatever
// the compiler makes of it (v_fma_f32 / v_pk_fma_f32), then one conversion.  fp16: v_fma_mixlo_f16 by hand — the sum is rounded once,
// straight to 16 bits: two kernels of one plan (gett_h16w4x_kernel / gett_h16w4p_kernel) differed in the last bit of a few results per
// million while the compiler chose (profiles/r06w, r06x).
template <bool BF>
__device__ __forceinline__ uint16_t h_round16_with_c(float v, float beta, uint16_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (BF) return h_round16<true>(__builtin_fmaf(beta, __uint_as_float((uint32_t)c << 16), v));
    else {
        uint32_t r;
        const uint32_t cw = c;
        asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(beta), "v"(cw), "v"(v));
        return (uint16_t)r;
    }
#else
    (void)v; (void)beta; (void)c; return 0;
#endif
}

}  // namespace ctamd
