// gett_gen_f64x.hip — instantiations of the single-precision-compute fp64 / complex128 GETT kernel (gett_gen_f64x.inc): operands rounded
// to fp32 / complex64 on their way into LDS, fp32 MFMA and accumulators, fp64 epilogue; and the fold of its fp32 split-K partials.
//   fp64:       V = 2 (16-byte loads of two fp64 on both operands) and V = 1 (8-byte gathers, any strides at all), 128 x 128 x 32 and
//               64 x 64 x 32 tiles each — 64 KiB / 32 KiB of static LDS
//   complex128: V = 1 (one element = one 16-byte load), 128 x 64 x 16 and 64 x 64 x 16 — 48 KiB / 32 KiB
#include "gett_gen_f64x.inc"

namespace ctamd {

static const GettKernelInfo g_gen_f64x_table[] = {
    CTAMD_F64X_ORIENTS(GEN_F64_F32, 128, 128, 32, 2)
    CTAMD_F64X_ORIENTS(GEN_F64_F32, 64, 64, 32, 2)
    CTAMD_F64X_ORIENTS(GEN_F64_F32, 128, 128, 32, 1)
    CTAMD_F64X_ORIENTS(GEN_F64_F32, 64, 64, 32, 1)
    CTAMD_F64X_ORIENTS(GEN_C64_C32, 128, 64, 16, 1)
    CTAMD_F64X_ORIENTS(GEN_C64_C32, 64, 64, 16, 1)
};

const GettKernelInfo* gett_gen_f64x_kernels(int* count) {
    *count = (int)(sizeof(g_gen_f64x_table) / sizeof(g_gen_f64x_table[0]));
    return g_gen_f64x_table;
}

// ---------------------------------------------------------------------------------------------
// Split-K fold of the kernels above: fp32 (complex: float2) partials [slice][L][M][N], one lane per output element (n fastest), the
// slices summed in sequence IN FP64, D = alpha * sum + beta * op(C) in fp64 on fp64 C / D.
// ---------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ void __launch_bounds__(256) gen_f64x_splitk_reduce_kernel(const SplitKReduceParams p) {
    constexpr int W = CPLX ? 2 : 1;
    const uint32_t Mtot = p.gM.total, Ntot = p.gN.total;
    const size_t plane = (size_t)Mtot * Ntot, total = plane * p.gL.total;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float* src = p.partial + e * W;
    double re = 0.0, im = 0.0;
    for (uint32_t s = 0; s < p.splitK; ++s) {
        re += (double)src[(size_t)s * total * W];
        if constexpr (CPLX) im += (double)src[(size_t)s * total * W + 1];
    }
    const uint32_t l = (uint32_t)(e / plane);
    const size_t rem = e - (size_t)l * plane;
    const uint32_t m = (uint32_t)(rem / Ntot), n = (uint32_t)(rem - (size_t)m * Ntot);
    int64_t oDl, oCl, oDm, oCm, oDn, oCn;
    group_offset2<2>(p.gL, p.cStrideL, l, oDl, oCl);
    group_offset2<1>(p.gM, p.cStrideM, m, oDm, oCm);
    group_offset2<1>(p.gN, p.cStrideN, n, oDn, oCn);
    const int64_t oD = oDl + oDm + oDn, oC = oCl + oCm + oCn;
    const double alRe = p.alpha64, alIm = p.alphaIm, beRe = p.beta64, beIm = p.betaIm;
    if constexpr (!CPLX) {
        double val = alRe * re;
        if (beRe != 0.0) val += beRe * static_cast<const double*>(p.C)[oC];
        static_cast<double*>(p.D)[oD] = val;
    } else {
        double oRe = alRe * re, oIm = alRe * im;      // (a real alpha scales: no 0 * inf)
        if (alIm != 0.0) { oRe -= alIm * im; oIm += alIm * re; }
        if (beRe != 0.0 || beIm != 0.0) {
            const double* c = static_cast<const double*>(p.C) + 2 * oC;
            const double cRe = c[0], cIm = p.conjC ? -c[1] : c[1];
            oRe += beRe * cRe - beIm * cIm;
            oIm += beRe * cIm + beIm * cRe;
        }
        double* d = static_cast<double*>(p.D) + 2 * oD;
        d[0] = oRe;
        d[1] = oIm;
    }
}

hipError_t launch_gen_f64x_splitk_reduce(const SplitKReduceParams& p, int elem, hipStream_t stream) {
    const size_t total = (size_t)p.gM.total * p.gN.total * p.gL.total;
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    switch (elem) {
        case GEN_F64_F32: hipLaunchKernelGGL((gen_f64x_splitk_reduce_kernel<false>), grid, block, 0, stream, p); break;
        case GEN_C64_C32: hipLaunchKernelGGL((gen_f64x_splitk_reduce_kernel<true>), grid, block, 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ctamd
