// gett_gen_c32x.hip — instantiations of the reduced-precision complex64 GETT kernel (gett_gen_c32x.inc): complex64 data, real and
// imaginary parts rounded to bf16 / fp16 (or split into two bf16 planes each for TF32) on their way into LDS, four (twelve) 16-bit
// MFMAs per complex product, fp32 accumulators and complex epilogue.
//   V = 2: 16-byte loads of two complex64 on both operands, any K extent (ragged last K-tile), any M / N — 128 x 128 and 64 x 64 tiles
//   V = 1: 8-byte gathers, any strides at all
// K-tiles are 32 deep: two 16-bit images per operand (16BF, 16F) are 64 KiB of static LDS for the 128 x 128 tile, four (TF32) 128 KiB.
#include "gett_gen_c32x.inc"

namespace ctamd {

#define CTAMD_C32X_MODE(GE)                   \
    CTAMD_C32X_ORIENTS(GE, 128, 128, 32, 2)   \
    CTAMD_C32X_ORIENTS(GE, 64, 64, 32, 2)     \
    CTAMD_C32X_ORIENTS(GE, 128, 128, 32, 1)   \
    CTAMD_C32X_ORIENTS(GE, 64, 64, 32, 1)

static const GettKernelInfo g_gen_c32x_table[] = {CTAMD_C32X_MODE(GEN_C32_BF16) CTAMD_C32X_MODE(GEN_C32_F16) CTAMD_C32X_MODE(GEN_C32_BF16X3)};

const GettKernelInfo* gett_gen_c32x_kernels(int* count) {
    *count = (int)(sizeof(g_gen_c32x_table) / sizeof(g_gen_c32x_table[0]));
    return g_gen_c32x_table;
}

}  // namespace ctamd
