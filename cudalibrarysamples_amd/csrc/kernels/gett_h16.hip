// gett_h16.hip — the merged kernel table of the aligned bf16 / fp16 GETT family, and the MFMA-ceiling measurement.
//
// The family's kernels live in gett_h16v.hip (the default gett_h16w4x_kernel and its 128 x 128 / 64 x 64 siblings) and gett_h16p.hip
// (the persistent 256 x 256 kernel); their shared pieces are gett_h16_common.h / gett_h16x_common.h.  This file holds
//   * gett_h16_kernels(): the family's one table, in the order of H16Variant (launch.h).  Its first 40 entries are the slots of
//     the five kernel families that were this file's content until round 5 (gett_h16_kernel: eight waves in two ping-pong rows;
//     gett_h16w4_kernel; the streamed gett_h16s_kernel / gett_h16w4s_kernel; the register-staged gett_h16w4r_kernel).  The kernels
//     are gone, the slots stay: kernel indices are written into plan-cache files, so the table keeps its length and order.  A slot
//     of a retired family has `ablation` = 2 ("not built"), which rank_h16_choices skips, and a launcher that answers
//     hipErrorNotSupported.
//   * ctamdMeasureMfmaCeiling[Shape]: the rate at which this device sustains nothing but MFMAs, which bench.py quotes the GETT
//     kernels against.
#include "gett_h16_common.h"

namespace ctamd {

// ---------------------------------------------------------------------------------------------------------------------
// Measurement only: the rate at which THIS device sustains nothing but independent v_mfma_f32_32x32x16_{bf16,f16} on a
// given kind of operand data (one wave per SIMD, eight operand register pairs, no memory traffic at all).  On zeros it
// is the nominal peak; on U(-1,1) data the power limit pulls the clock down and the rate differs from box to box by up to
// 30 % — bench.py quotes the GETT kernel against both.
// ---------------------------------------------------------------------------------------------------------------------
template <bool BF>
__global__ void __launch_bounds__(256, 1) mfma_ceiling_kernel(const s16x8* __restrict__ data, float* out, int iters) {
    s16x8 a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = data[(i * 2 + 0) * 256 + threadIdx.x];
        b[i] = data[(i * 2 + 1) * 256 + threadIdx.x];
    }
    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i & 7] = h_mfma<BF>(a[i & 7], b[(i >> 1) & 7], acc[i & 7]);
    }
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) r += acc[i][0] + acc[i][7];
    out[blockIdx.x * 256 + threadIdx.x] = r;
}

// the same for v_mfma_f32_16x16x32_{bf16,f16} (the default 16-bit kernel's instruction, gett_h16v.hip), issued from inline asm like there
template <bool BF>
__global__ void __launch_bounds__(256, 1) mfma16_ceiling_kernel(const s16x8* __restrict__ data, float* out, int iters) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    s16x8 a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = data[(i * 2 + 0) * 256 + threadIdx.x];
        b[i] = data[(i * 2 + 1) * 256 + threadIdx.x];
    }
    f32x4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {   // 32 x (16x16x32) = the flops of 16 x (32x32x16)
#if defined(__HIP_DEVICE_COMPILE__)
            if constexpr (BF) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i & 15]) : "v"(a[i & 7]), "v"(b[(i >> 1) & 7]));
            else              asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc[i & 15]) : "v"(a[i & 7]), "v"(b[(i >> 1) & 7]));
#endif
        }
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) r += acc[i][0] + acc[i][3];
    out[blockIdx.x * 256 + threadIdx.x] = r;
}

}  // namespace ctamd

// dataKind 0: zeros, 1: U(-1,1) (fixed seed); shape 0: 32x32x16, 1: 16x16x32.  Returns 0 and the sustained TFLOP/s (after ~40 ms of
// burn-in), or -1.
extern "C" int ctamdMeasureMfmaCeilingShape(int bf16, int dataKind, int shape, float* tflops);
extern "C" int ctamdMeasureMfmaCeiling(int bf16, int dataKind, float* tflops) { return ctamdMeasureMfmaCeilingShape(bf16, dataKind, 0, tflops); }
extern "C" int ctamdMeasureMfmaCeilingShape(int bf16, int dataKind, int shape, float* tflops) {
    using namespace ctamd;
    if (tflops == nullptr) return -1;
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    const int cus = prop.multiProcessorCount;
    const size_t n = 16 * 256 * 8;     // 8 operand pairs x 256 lanes x 8 elements
    uint16_t* h = static_cast<uint16_t*>(malloc(n * 2));
    if (h == nullptr) return -1;
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        const float x = dataKind == 0 ? 0.f : 2.f * (float)(lcg >> 8) / 16777216.f - 1.f;
        if (bf16) {
            uint32_t u;
            memcpy(&u, &x, 4);
            u += 0x7fffu + ((u >> 16) & 1u);
            h[i] = (uint16_t)(u >> 16);
        } else {
            const _Float16 hf = (_Float16)x;
            memcpy(&h[i], &hf, 2);
        }
    }
    s16x8* d = nullptr;
    float* out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = -1;
    if (hipMalloc((void**)&d, n * 2) == hipSuccess && hipMalloc((void**)&out, (size_t)cus * 256 * 4) == hipSuccess &&
        hipMemcpy(d, h, n * 2, hipMemcpyHostToDevice) == hipSuccess && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
        const int iters = 20000;       // ~12-25 ms per launch
        auto launch = [&]() {
            if (shape == 1) {
                if (bf16) hipLaunchKernelGGL((mfma16_ceiling_kernel<true>), dim3(cus), dim3(256), 0, nullptr, d, out, iters);
                else      hipLaunchKernelGGL((mfma16_ceiling_kernel<false>), dim3(cus), dim3(256), 0, nullptr, d, out, iters);
            } else {
                if (bf16) hipLaunchKernelGGL((mfma_ceiling_kernel<true>), dim3(cus), dim3(256), 0, nullptr, d, out, iters);
                else      hipLaunchKernelGGL((mfma_ceiling_kernel<false>), dim3(cus), dim3(256), 0, nullptr, d, out, iters);
            }
        };
        for (int w = 0; w < 3; ++w) launch();
        (void)hipEventRecord(e0, nullptr);
        for (int w = 0; w < 3; ++w) launch();
        (void)hipEventRecord(e1, nullptr);
        float ms = 0.f;
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.f) {
            const double flops = 3.0 * (double)cus * 4 * iters * 16 * 2.0 * 32 * 32 * 16;
            *tflops = (float)(flops / (ms * 1e-3) / 1e12);
            rc = 0;
        }
    }
    (void)hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (out) (void)hipFree(out);
    free(h);
    return rc;
}

namespace ctamd {

// the slots of the five families retired from this file (CTAMD_H16_RETIRED8: gett_h16_common.h)
static const GettKernelInfo g_h16_table[] = {
    CTAMD_H16_RETIRED8(kHBK, 4, 512, 5, "gett_h16_kernel", H16_W8)         // eight waves in two ping-pong rows
    CTAMD_H16_RETIRED8(kHBK, 2, 256, 2, "gett_h16w4_kernel", H16_W4)       // four waves, one per SIMD
    CTAMD_H16_RETIRED8(32, 4, 512, 4, "gett_h16s_kernel", H16_S)           // eight free-running waves on a K-tile-32 ring
    CTAMD_H16_RETIRED8(32, 2, 256, 5, "gett_h16w4s_kernel", H16_W4S)       // four free-running waves on the same ring
    CTAMD_H16_RETIRED8(kHBK, 2, 256, 3, "gett_h16w4r_kernel", H16_W4R)};   // four waves, register-staged (no LDS-DMA)

// The whole family in the order of H16Variant (launch.h), which names each variant's first entry: this file's five, then gett_h16v.hip's
// table (H16_W4V: one more retired slot, H16_W4X: the default 256 x 256 kernel, H16_W4M / H16_W4M4 / H16_W8M: the 128 x 128 tile, H16_W4Q: the
// 64 x 64 tile), then H16_W4P, the persistent 256 x 256 kernel (gett_h16p.hip, round 5); eight entries each, same order
const GettKernelInfo* gett_h16_kernels(int* count) {
    constexpr int nHere = (int)(sizeof(g_h16_table) / sizeof(g_h16_table[0]));
    struct All { GettKernelInfo e[nHere + 56 + 8]; int n; };
    static const All all = [] {
        All a{};
        for (int i = 0; i < nHere; ++i) a.e[i] = g_h16_table[i];
        int nv = 0;
        const GettKernelInfo* v = gett_h16v_kernels(&nv);
        a.n = nHere;
        for (int i = 0; i < nv && i < 56; ++i) a.e[a.n++] = v[i];
        const GettKernelInfo* pk = gett_h16p_kernels(&nv);     // H16_W4P: the persistent 256 x 256 kernel (gett_h16p.hip)
        for (int i = 0; i < nv && i < 8; ++i) a.e[a.n++] = pk[i];
        return a;
    }();
    *count = all.n;
    return all.e;
}

}  // namespace ctamd
