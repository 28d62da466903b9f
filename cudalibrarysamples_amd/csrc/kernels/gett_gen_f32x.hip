// gett_gen_f32x.hip — instantiations of the reduced-precision fp32 GETT kernel (gett_gen_f32x.inc): fp32 data, operands rounded to
// bf16 / fp16 (or split into two bf16 planes for TF32) on their way into LDS, fp32 accumulators and epilogue.
//   V = 4: 16-byte loads of four fp32 on both operands, any K extent (ragged last K-tile), any M / N — 128 x 128 and 64 x 64 tiles
//   V = 1: 4-byte gathers, any strides at all
// K-tiles: 64 deep with one 16-bit image per operand (16BF, 16F at V = 4), 32 deep with two (TF32) and for the gathers — 64 KiB of
// static LDS for the 128 x 128 tile either way.
#include "gett_gen_f32x.inc"

namespace ctamd {

static const GettKernelInfo g_gen_f32x_table[] = {
    CTAMD_F32X_ORIENTS(GEN_F32_BF16, 128, 128, 64, 4)
    CTAMD_F32X_ORIENTS(GEN_F32_BF16, 64, 64, 64, 4)
    CTAMD_F32X_ORIENTS(GEN_F32_BF16, 128, 128, 32, 1)
    CTAMD_F32X_ORIENTS(GEN_F32_BF16, 64, 64, 32, 1)
    CTAMD_F32X_ORIENTS(GEN_F32_F16, 128, 128, 64, 4)
    CTAMD_F32X_ORIENTS(GEN_F32_F16, 64, 64, 64, 4)
    CTAMD_F32X_ORIENTS(GEN_F32_F16, 128, 128, 32, 1)
    CTAMD_F32X_ORIENTS(GEN_F32_F16, 64, 64, 32, 1)
    CTAMD_F32X_ORIENTS(GEN_F32_BF16X3, 128, 128, 32, 4)
    CTAMD_F32X_ORIENTS(GEN_F32_BF16X3, 64, 64, 32, 4)
    CTAMD_F32X_ORIENTS(GEN_F32_BF16X3, 128, 128, 32, 1)
    CTAMD_F32X_ORIENTS(GEN_F32_BF16X3, 64, 64, 32, 1)
};

const GettKernelInfo* gett_gen_f32x_kernels(int* count) {
    *count = (int)(sizeof(g_gen_f32x_table) / sizeof(g_gen_f32x_table[0]));
    return g_gen_f32x_table;
}

}  // namespace ctamd
