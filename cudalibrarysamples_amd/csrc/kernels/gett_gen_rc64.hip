// gett_gen_rc64.hip — instantiations of the mixed fp64 x complex128 kernel of the general MFMA family (gett_gen_rc64.inc): 64 x 64 x 8,
// the real operand as kernel-A (side 0) or kernel-B (side 1), at 16-byte lanes (V = 2) or 8-byte gathers (V = 1); the complex operand
// always loads single 16-byte elements.  Appended to the family's table behind every earlier row (gett_gen_kernels, gett_gen_h16.hip).
#include "gett_gen_rc64.inc"

namespace ctamd {

static const GettKernelInfo g_gen_rc64_table[] = {
    CTAMD_GEN_RC64_ORIENTS(0, 2)
    CTAMD_GEN_RC64_ORIENTS(0, 1)
    CTAMD_GEN_RC64_ORIENTS(1, 2)
    CTAMD_GEN_RC64_ORIENTS(1, 1)};

const GettKernelInfo* gett_gen_rc64_kernels(int* count) {
    *count = (int)(sizeof(g_gen_rc64_table) / sizeof(g_gen_rc64_table[0]));
    return g_gen_rc64_table;
}

}  // namespace ctamd
