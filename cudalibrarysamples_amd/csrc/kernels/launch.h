// launch.h — host-visible launch interface of the gfx950 kernels (implemented in the .hip files).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>

#include "params.h"

namespace ctamd {

enum OperandLayout : int {
    LAY_F = 0,  // fastest free mode has stride 1: 16-byte lanes along rows
    LAY_K = 1,  // fastest contracted mode has stride 1: 16-byte lanes along k
    LAY_S = 2   // arbitrary strides: 4-byte gathers
};

// Variants of the aligned 16-bit family, gett_h16<name>_kernel.  gett_h16_kernels() holds eight entries per variant — bf16 first, then
// fp16, each in the order (layA, layB) = (K,K) (K,F) (F,K) (F,F) — and a variant's value is the table position of its first entry: the
// table's order and length are fixed (kernel indices are written into plan-cache files), and this is where the order is written down.
enum H16Variant : int {
    H16_W8 = 0, H16_W4 = 8, H16_S = 16, H16_W4S = 24, H16_W4R = 32, H16_W4V = 40,   // retired families (slots without kernels): eight waves
                     // in two ping-pong rows; four waves, one per SIMD; eight / four free-running waves on a K-tile-32 ring; four waves
                     // register-staged; four waves with the lean instruction stream on the 32x32x16 MFMA
    H16_W4X  = 48,   // the lean four-wave kernel on the 16x16x32 MFMA: the default 256 x 256 kernel
    H16_W4M  = 56,   // 128 x 128 on a two-deep ring, two workgroups per CU
    H16_W4M4 = 64,   // 128 x 128 on a four-deep ring, one workgroup per CU
    H16_W8M  = 72,   // 128 x 128, four multiplying + four data-moving waves
    H16_W4Q  = 80,   // 64 x 64, two workgroups per CU (also the strip kernel of a strip plan)
    H16_W4P  = 88    // the persistent 256 x 256 kernel (gett_h16p.hip); its one-tile twin is H16_W4X
};
constexpr int h16_entry(H16Variant variant, int layoutIdx) { return (int)variant + layoutIdx; }   // layoutIdx 0..7

struct GettKernelInfo {
    int bm, bn, bk;      // workgroup tile
    int wm, wn, wk;      // wave grid inside the workgroup
    int layA, layB;      // OperandLayout of kernel-A / kernel-B
    int threads;
    int pf;              // fp32 family: K-tiles in flight (registers, or the depth of the LDS ring); 16-bit and general families: a code
                         // that tools read from ctamdDescribePlan and nothing in the library tests — identity is `name` / `variant`
    int kfast;           // 1: requires extent(fastest K mode) % bk == 0
    int ablation;        // != 0: measurement-only variant (wrong results), never ranked by default
    hipError_t (*launch)(const GettParams&, hipStream_t);
    int fragPartials;    // 1: split-K partials are written in accumulator order (padded tiles), folded by
                         //    launch_splitk_reduce_frag; 0: row-major [M][N], launch_splitk_reduce
    int nt;              // 1: operands are streamed with the nontemporal policy (no Infinity-Cache allocation): ranked only for
                         //    problems that read every operand byte once and whose operands exceed the Infinity Cache anyway
    int elem;            // general family (gett_gen_kernels): GenElem of the instantiation
    int vec;             // general family: elements per staged unit = per global load (both operands; GEN_RC64: the real operand's — the
                         // complex one always loads single 16-byte elements)
    const char* name;    // the __global__ template the entry launches (ctamdDescribePlan's "kname")
    int variant;         // aligned 16-bit family: H16Variant of the entry (0 in the other families' tables, but for the GEN_RC64 rows of the
                         // general family: which kernel operand is the real one — 0 kernel-A, 1 kernel-B)
};

// element types of the general MFMA family (gett_gen.inc)
enum GenElem : int { GEN_BF16 = 0, GEN_F16 = 1, GEN_F64 = 2, GEN_C32 = 3, GEN_C64 = 4,
                     // fp32 DATA under a reduced-precision compute descriptor (gett_gen_f32x.inc): operands rounded to bf16 / fp16, or split
                     // into two bf16 planes (three products: COMPUTE_DESC_TF32), on their way into LDS; fp32 accumulators, partials, epilogue
                     GEN_F32_BF16 = 5, GEN_F32_F16 = 6, GEN_F32_BF16X3 = 7,
                     // fp64 / complex128 DATA under COMPUTE_DESC_32F (gett_gen_f64x.inc): operands rounded to fp32 / complex64 on their way
                     // into LDS, fp32 MFMA and accumulators, fp32 / float2 partials, fp64 epilogue and fold
                     GEN_F64_F32 = 8, GEN_C64_C32 = 9,
                     // complex64 DATA under a reduced-precision compute descriptor (gett_gen_c32x.inc): real and imaginary parts rounded to
                     // bf16 / fp16, or split into two bf16 planes each (COMPUTE_DESC_TF32), on their way into LDS; four (twelve) 16-bit MFMAs per
                     // complex product; fp32 accumulators, float2 partials and the complex64 epilogue and fold of GEN_C32
                     GEN_C32_BF16 = 10, GEN_C32_F16 = 11, GEN_C32_BF16X3 = 12,
                     // one real fp64 operand, the other one and C / D complex128 (gett_gen_rc64.inc): two fp64 MFMAs per product into two
                     // accumulators (re, im), double2 partials and the complex128 epilogue and fold of GEN_C64
                     GEN_RC64 = kGenElemRC64 };
inline bool gen_elem_is_f32x(int elem) { return elem >= GEN_F32_BF16 && elem <= GEN_F32_BF16X3; }
inline bool gen_elem_is_f64x(int elem) { return elem == GEN_F64_F32 || elem == GEN_C64_C32; }
inline bool gen_elem_is_c32x(int elem) { return elem >= GEN_C32_BF16 && elem <= GEN_C32_BF16X3; }
// split-K partials of the element type are fp32 rows folded by launch_splitk_reduce (else: launch_gen_splitk_reduce — the fp32 / float2
// partials of the gen_elem_is_f64x elements among them, whose fold is in fp64)
inline bool gen_elem_f32_partials(int elem) { return elem == GEN_BF16 || elem == GEN_F16 || gen_elem_is_f32x(elem); }
// bytes of one split-K partial element
inline unsigned gen_elem_partial_bytes(int elem) {
    return (gen_elem_f32_partials(elem) || elem == GEN_F64_F32) ? 4u : (elem == GEN_C64 || elem == GEN_RC64) ? 16u : 8u;
}

// fp32 data, fp32 MFMA (v_mfma_f32_16x16x4_f32)
const GettKernelInfo* gett_f32_kernels(int* count);
hipError_t launch_splitk_reduce(const SplitKReduceParams& p, hipStream_t stream);
hipError_t launch_splitk_reduce_frag(const SplitKReduceParams& p, hipStream_t stream);
// streaming (LDS-DMA ring) kernels, gett_f32_stream.hip; gett_f32_kernels() returns the merged table
const GettKernelInfo* gett_f32_stream_kernels(int* count);
extern std::atomic<uint64_t> g_flatStartLaunches;   // launches of those kernels that took a flat entry (StreamFlatParams, or scalar parameters)

// bf16 / fp16 data, fp32 accumulation (v_mfma_f32_16x16x32_{bf16,f16}): the merged table, gett_h16.hip
const GettKernelInfo* gett_h16_kernels(int* count);
const GettKernelInfo* gett_h16v_kernels(int* count);   // gett_h16v.hip: appended to the table above, H16_W4V .. H16_W4Q
const GettKernelInfo* gett_h16p_kernels(int* count);   // gett_h16p.hip (persistent 256 x 256 kernel): H16_W4P

// general MFMA family: bf16 / fp16 shapes the aligned kernels above refuse (no 16-byte lanes, K not in whole 64-deep tiles), fp64,
// complex64 / complex128 — register-staged, any strides and extents (gett_gen.inc; the table is the concatenation of the three
// translation units gett_gen_h16.hip / gett_gen_f64.hip / gett_gen_cplx.hip, then — appended, so that every earlier index stays — the
// reduced-precision fp32 kernels of gett_gen_f32x.hip, then the single-precision-compute fp64 / complex128 kernels of gett_gen_f64x.hip,
// then the reduced-precision complex64 kernels of gett_gen_c32x.hip, then the mixed fp64 x complex128 kernels of gett_gen_rc64.hip)
const GettKernelInfo* gett_gen_kernels(int* count);
const GettKernelInfo* gett_gen_h16_kernels(int* count);
const GettKernelInfo* gett_gen_f64_kernels(int* count);
const GettKernelInfo* gett_gen_cplx_kernels(int* count);
const GettKernelInfo* gett_gen_f32x_kernels(int* count);
const GettKernelInfo* gett_gen_f64x_kernels(int* count);
const GettKernelInfo* gett_gen_c32x_kernels(int* count);
const GettKernelInfo* gett_gen_rc64_kernels(int* count);
// split-K fold of the general family's fp64 / complex kernels: D = alpha * sum_s partial[s] + beta * op(C); partials
// [slice][L][M][N] in the accumulator type of `elem` (GEN_F64: double, GEN_C32 and GEN_C32_BF16 / _F16 / _BF16X3: float2, GEN_C64: double2; GEN_F64_F32: float and
// GEN_C64_C32: float2, summed and scaled in fp64 on fp64 C / D — gett_gen_f64x.hip; GEN_RC64: double2, folded as GEN_C64)
hipError_t launch_gen_splitk_reduce(const SplitKReduceParams& p, int elem, hipStream_t stream);
hipError_t launch_gen_f64x_splitk_reduce(const SplitKReduceParams& p, int elem, hipStream_t stream);

// simple one-thread-per-output contraction for every other dtype (and > kMaxGroupModes problems)
hipError_t launch_gett_simple(const GettParams& p, int dtype /*hipDataType*/, bool accumulate64,
                              hipStream_t stream);

// any number of modes (mode table in device memory), one output element per lane
hipError_t launch_gett_wide(const WideParams& p, int dtype /*hipDataType*/, bool accumulate64, hipStream_t stream);

// element-wise family (elementwise.hip)
enum EwVariant : int {
    EW_TRANSPOSE = 0,  // sD0 == 1 and sA1 == 1: 64x64 LDS tile, 16-byte lanes on both sides
    EW_ROWCOPY   = 1,  // sD0 == 1 and sA0 == 1: 16-byte lanes along dim0, no LDS
    EW_GENERIC   = 2,  // any strides, any dtype: one element per lane
    EW_TRANSPOSE_ANY = 4,  // pure permutation of 2- / 4-byte elements, D contiguous along dim0 and A along dim1, any extents / alignment: 64 x 64 LDS tile, element-wise
    EW_BLOCK     = 3,  // pure permutation of 2- / 4-byte elements whose leading modes are the same packed set in A and D: contiguous blocks
                       // through LDS, permuted inside (Ew2DParams::blk*); falls back to EW_GENERIC when a C / E / X operand is attached
    // more unfusable modes than Ew2DParams describes (elementwise_table.hip, on an EwTable instead):
    EW_TABLE_TILE   = 5,   // A and D each have a stride-1 mode, A carries every mode of D: tiles through LDS, read in A's order, written in D's
    EW_TABLE_GATHER = 6    // anything else: one output element per lane, every digit decoded
};
// Grid of a tiled element-wise launch.  One workgroup per tile: a workgroup that loops over tiles serialises its own read -> barrier ->
// write phases, fresh workgroups overlap them across the CU (2048^3 permutation, 64 x 64 tiles: 5.37 TB/s with the grid capped at 32 Ki
// workgroups, 6.09-6.14 with one workgroup per tile; profiles/r03_transpose_sweep*.jsonl).  Under tile order 1 the transposing kernels
// walk 8 * idsPerXcd ids; the grid-stride loops stay for tensors beyond 2^22 tiles.
inline unsigned ew_tiled_grid(const Ew2DParams& p, int variant) {
    const unsigned grid = (variant == EW_TRANSPOSE && p.order) ? 8u * p.idsPerXcd : p.nBlocks;
    return grid > (1u << 22) ? (1u << 22) : grid;
}
hipError_t launch_elementwise(const Ew2DParams& p, int variant, int dtype, hipStream_t stream);
// the converting kernels (elementwise_convert.hip): A of dtypeA, D and C of dtypeD — bf16 / fp16 <-> fp32 and fp32 <-> fp64; variants
// EW_TRANSPOSE / EW_ROWCOPY / EW_GENERIC with a lane of 16 / min(sizeof A, sizeof D) elements; any other pair or variant is an error
hipError_t launch_elementwise_convert(const Ew2DParams& p, int variant, int dtypeA, int dtypeD, hipStream_t stream);
// the complex trinary kernels (elementwise_trinary_cplx.hip): complex64 / complex128 data with an E and / or X operand attached; variants
// EW_TRANSPOSE / EW_ROWCOPY / EW_GENERIC.  p carries the scalars' other parts (alpha64 / alphaIm, gamma64 / gammaIm, xi64, delta64) and
// conjA / conjC; Ew3CplxExtras is what Ew2DParams has no field for
struct Ew3CplxExtras {
    double  xiIm = 0.0, deltaIm = 0.0;   // imaginary parts of xi (X's scalar) and delta (E's scalar)
    int32_t conjX = 0, conjE = 0;
};
hipError_t launch_elementwise_trinary_cplx(const Ew2DParams& p, const Ew3CplxExtras& x, int variant, int dtype, hipStream_t stream);
// D[0 .. n) = value (contiguous; the padded-permutation border fill)
hipError_t launch_fill(void* D, uint64_t n, int dtype, double value, hipStream_t stream);

// reduction family (reduce.hip)
enum ReduceVariant : int {
    RED_COL     = 0,   // A's stride-1 mode is kept: lanes along it (float4), loop over reduced modes
    RED_ROW     = 1,   // A's stride-1 mode is reduced: one workgroup per kept element
    RED_GENERIC = 2,   // any strides, any dtype
    RED_TABLE   = 3    // a kept or reduced group of more than kMaxGroupModes digits (elementwise_table.hip, on an EwTable)
};
hipError_t launch_reduce(const ReduceParams& p, int variant, int dtype, bool acc64, hipStream_t stream);
hipError_t launch_reduce_finalize(const ReduceParams& p, int dtype, bool acc64, hipStream_t stream);

// the mode-table kernels (elementwise_table.hip; the table: ew_table_layout.h).  Element-wise: the tile or the gather kernel by
// EwTable::kind on `grid` workgroups, each looping over tiles / elements.  Reduction: reduce_table_kernel and, when the table carries
// partials (splitR > 1), reduce_table_finalize_kernel behind it.
struct EwTable;
hipError_t launch_elementwise_table(const EwTable& t, int dtype, unsigned grid, hipStream_t stream);
hipError_t launch_reduce_table(const EwTable& t, int dtype, bool acc64, hipStream_t stream);

}  // namespace ctamd
