// internal.hpp — objects behind the opaque cuTENSOR handles and the planner interfaces.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <cutensor.h>

#include "api_guard.hpp"
#include "plan_store.hpp"

// Every behaviour-changing environment switch of this library is read through CTAMD_HOOK_ENV (api_guard.hpp): live in the test-hooks
// flavour (lib_hooks/), a null pointer in the production library.  That covers the switches the test-suite drives behaviour with
// (CUTENSOR_AMD_GEN, _PEEL, _NT, _FUSED_FOLD, _H16_WAVES, _H16P, ...) and the measurement-only ones (CUTENSOR_AMD_FORCE, _XCD_BALANCE,
// _KORDER, _ABLATION, _H16_SPLITK, _H16_TRANSPOSE_T1).  The production library reads CUTENSOR_LOG_LEVEL and nothing else.
#include "../kernels/launch.h"
#include "../kernels/params.h"
#include "../kernels/ew_table_layout.h"

// The ABI names these structs only as opaque pointer targets (cutensor/types.h).
struct cutensorComputeDescriptor {
    int      id;          // index into the exported constants
    uint32_t legacyBits;  // cutensorComputeType_t value (Mg entry points)
};

struct cutensorTensorDescriptor {
    uint32_t             numModes = 0;
    std::vector<int64_t> extent;
    std::vector<int64_t> stride;
    hipDataType          dtype = HIP_R_32F;
    uint32_t             alignment = 0;
    int64_t numElementsSpanned() const { int64_t n = 1; for (uint32_t i = 0; i < numModes; ++i) n += (extent[i] - 1) * stride[i]; return n; }   // 1 + sum (extent-1)*stride
};

enum class OpKind : int { Contraction = 0, Reduction = 1, Permutation = 2, ElementwiseBinary = 3, ElementwiseTrinary = 4,
                           ContractionTrinary = 5, BlockSparseContraction = 6 };

struct TensorUse {
    cutensorTensorDescriptor desc;
    std::vector<int32_t>     modes;
    cutensorOperator_t       op = CUTENSOR_OP_IDENTITY;
    bool                     present = false;
};

namespace ctamd { struct BlockSparseOp; struct BlockSparsePlan; }

struct cutensorOperationDescriptor {
    OpKind      kind;
    std::shared_ptr<ctamd::BlockSparseOp> bs;        // block-sparse contraction (host/blocksparse.cpp)
    TensorUse   A, B, C, D;
    TensorUse   E;                                   // output of a trinary contraction (D is its beta source)
    cutensorOperator_t opReduce = CUTENSOR_OP_ADD;   // reduction operator / binary combiner (opAC, opABC)
    cutensorOperator_t opAB = CUTENSOR_OP_ADD;       // element-wise trinary: first combiner
    const cutensorComputeDescriptor* compute = nullptr;
    hipDataType scalarType = HIP_R_32F;
    int32_t     tag = 0;
    // trinary contraction E = alpha A B C + beta D (contraction_trinary.cu:191-198) as two pairwise contractions:
    // sub[0]: T = X * Y (packed intermediate in the workspace), sub[1]: E = alpha T * Z + beta D
    std::vector<cutensorOperationDescriptor> sub;
    int         triOrder[3] = {0, 1, 2};   // operand indices (0 = A, 1 = B, 2 = C) playing X, Y, Z
    uint64_t    tBytes = 0;
    // CUTENSOR_OPERATION_DESCRIPTOR_PADDING_{LEFT,RIGHT,VALUE} of a permutation (elementwise_permute_padding.cu:178-195)
    std::vector<int32_t> padLeft, padRight;
    double      padValue = 0.0;
    double      flops = 0.0;
    double      movedBytes = 0.0;
};

struct cutensorPlanPreference {
    cutensorAlgo_t         algo = CUTENSOR_ALGO_DEFAULT;
    cutensorJitMode_t      jit = CUTENSOR_JIT_MODE_NONE;
    cutensorAutotuneMode_t autotune = CUTENSOR_AUTOTUNE_MODE_NONE;
    cutensorCacheMode_t    cacheMode = CUTENSOR_CACHE_MODE_PEDANTIC;
    int32_t                incrementalCount = 4;
    int32_t                kernelRank = 0;
    int32_t                operandsStreamed = 0;   // CUTENSOR_AMD_PLAN_PREFERENCE_OPERANDS_STREAMED (engine extension)
};

namespace ctamd {

// ---- contraction planning --------------------------------------------------------------------
struct CanonMode {
    int32_t label;
    int64_t extent;
    int64_t sA = 0, sB = 0, sC = 0, sD = 0;   // element strides (kernel-A / kernel-B / C / D)
};

struct ContractionView {
    std::vector<CanonMode> L, M, N, K;   // fused, fastest first
    bool     swapped = false;            // kernel-A is the user's B
    int      layA = LAY_S, layB = LAY_S; // best layout each operand admits
    hipDataType dtype = HIP_R_32F;
    uint64_t totL = 1, totM = 1, totN = 1, totK = 1;
    bool     wide = false;               // a group has more than kMaxGroupModes unfusable modes (or >= 2^31 elements):
                                         // only the mode-table kernel (gett_wide_kernel) can run it
    bool     lanesA = false, lanesB = false;   // fp32: the operand has 16-byte lanes in the strict sense (pointer, extent of the stride-1
                                         // mode and every other stride multiples of 16 bytes) — what the register-staged kernels
                                         // (gett_f32.hip) need; the LDS-DMA ring kernels take layA / layB as they are (round 6)
    uint32_t alignA = 0, alignB = 0;     // descriptor alignment (bytes) of kernel-A / kernel-B
    uint32_t alignD = 0;                 // ... of the output
    // The mixed rows of the type table (one input real fp64, the other one, C and D complex128): which KERNEL operand is the real one —
    // 0 kernel-A, 1 kernel-B; -1: both inputs have `dtype`.  `dtype` stays the output's type; byte sizes, alignment and vector widths
    // of an input come from type_of().
    int      realSide = -1;
    hipDataType type_of(bool slotA) const { return realSide == (slotA ? 0 : 1) ? HIP_R_64F : dtype; }
    // ... and which of the CALLER's inputs that is (0 = A, 1 = B; -1 none)
    int real_input() const { return realSide < 0 ? -1 : (realSide ^ (swapped ? 1 : 0)); }
};

// The shape of a contraction plan: what cutensorCreatePlan built and cutensorContract runs (cutensorPlan::planKind)
enum class PlanKind : int {
    Tiled,        // one launch of choice.kernel of choice.family (+ the split-K fold; + the strip launch of a strip plan)
    Simple,       // gett_simple_kernel: no family has a kernel for the problem
    ModeTable,    // gett_wide_kernel on cutensorPlan::wideTab
    Peeled,       // a host loop over cutensorPlan::peel around sub1 (sub2: the accumulate launches)
    LoneReduce,   // loneA / loneB reduce an operand over the modes it alone carries into a temporary, sub1 contracts the temporaries
    Repack        // loneA / loneB copy an operand into a packed temporary, sub1 contracts the temporaries
};

// One executable choice for a contraction.
struct ContractionChoice {
    int      kernel = -1;      // index into the family's kernel table; -1: none (PlanKind says what runs instead)
    int      family = 0;       // 0 = gett_f32_kernels() (fp32 data), 1 = gett_h16_kernels() (bf16 / fp16 data, aligned shapes),
                               // 2 = gett_gen_kernels() (general MFMA family: any 16-bit shape, fp64, complex; fp32 data under a reduced-precision compute descriptor)
    uint32_t splitK = 1;
    uint32_t kPerSlice = 0;
    uint64_t workspace = 0;
    double   estimateUs = 0.0;
    // Strip plan (16-bit family, pick_h16_choice): `kernel` covers only the interior [0, mInt) x [0, nInt) — whole tiles of its own size —
    // and ONE launch of table entry `stripKernel` (the 64 x 64 tile) covers the two edge strips, rows [mInt, M) x all columns and
    // rows [0, mInt) x columns [nInt, N).  4100^3 on 256 x 256 tiles is 17 x 17 = 289 tiles, two rounds on 256 CUs for 33 tiles that
    // hold four live rows or columns each; as 16 x 16 + strips it is one round plus ~20 us.  stripKernel < 0: none.
    int      stripKernel = -1;
    uint32_t mInt = 0, nInt = 0;
};

cutensorStatus_t build_contraction_view(const cutensorOperationDescriptor& op, ContractionView& v,
                                        std::string* why);
// Ranked candidate list (best first) under a workspace limit.
std::vector<ContractionChoice> rank_contraction_choices(const ContractionView& v, uint64_t wsLimit,
                                                        int numCUs, bool operandsStreamed = false);
// The order of the contracted digits a one-tile split-K plan of the streaming fp32 kernel runs on when exactly one operand is
// K-contiguous: that operand's stride-1 digit first, the others by the OTHER operand's strides.  True: `K` holds it and differs from v.K.
bool stream_k_order(const ContractionView& v, const ContractionChoice& c, std::vector<CanonMode>& K);
bool pick_h16_choice(const ContractionView& v, uint64_t wsLimit, int numCUs, ContractionChoice& c);
// general MFMA family (kernels/gett_gen.inc): false only for fp32 data and for views the tiled kernels cannot describe
// (f32xElem: fp32 data under a reduced-precision compute descriptor — GEN_F32_BF16 / GEN_F32_F16 / GEN_F32_BF16X3, gett_gen_f32x.inc)
// what f64x_decide compares: an fp64 / complex128 plan of the general family, or its single-precision twin, at its measured rate
double gen_f64_measured_estimate_us(const ContractionView& v, const ContractionChoice& c, int numCUs);
// (or fp64 / complex128 data under COMPUTE_DESC_32F — GEN_F64_F32 / GEN_C64_C32, gett_gen_f64x.inc)
// what f32x_decide compares on complex64 data: a complex64 plan of the general family, or its reduced-precision twin, at its measured rate
double gen_c32_measured_estimate_us(const ContractionView& v, const ContractionChoice& c, int numCUs);
// (or complex64 data under COMPUTE_DESC_16BF / _16F / _TF32 — GEN_C32_BF16 / GEN_C32_F16 / GEN_C32_BF16X3, gett_gen_c32x.inc)
bool pick_gen_choice(const ContractionView& v, uint64_t wsLimit, int numCUs, ContractionChoice& c, int f32xElem = -1);
// 16-bit family: the default kernel variant first, then the other variants of the same tile / split (the candidates
// CUTENSOR_ALGO_DEFAULT_PATIENT and incremental autotuning measure)
std::vector<ContractionChoice> rank_h16_choices(const ContractionView& v, uint64_t wsLimit, int numCUs);
int h16_waves_variant();   // the H16Variant CUTENSOR_AMD_H16_WAVES names (hooks flavour), else the default one
void fill_gett_params(const ContractionView& v, const ContractionChoice& c, GettParams& p,
                      SplitKReduceParams& r);

// ---- element-wise / reduction planning -------------------------------------------------------
struct EwPlan {
    int        variant = EW_GENERIC;
    Ew2DParams p{};              // pointers / scalars are filled at launch
    bool       usesC = false;
    bool       usesX = false;    // second permuted operand (trinary, both operands permuted)
    // variant EW_BLOCK: the variant the tile decomposition in p was laid out for (EW_GENERIC, or EW_TRANSPOSE when the block form was
    // preferred to mostly empty transposing tiles) — what runs when the block kernel cannot serve the launch (a unary operator on A)
    int        blockFrom = EW_GENERIC;
    // data types of A and of D (and C): they differ in a converting plan, which runs on kernels/elementwise_convert.hip
    hipDataType dtypeA = HIP_R_32F, dtypeD = HIP_R_32F;
    bool converts() const { return dtypeA != dtypeD; }
    // complex trinary plans (kernels/elementwise_trinary_cplx.hip): conjugation of the second permuted operand X and of the operand that
    // rides along as E — Ew2DParams, the argument block of the other kernels, has no field for either (run_elementwise hands them over
    // in an Ew3CplxExtras)
    int32_t    conjX = 0, conjE = 0;
    // variants EW_TABLE_TILE / EW_TABLE_GATHER (more unfusable modes than `p` describes; plan_elementwise_table.cpp): the mode table the
    // kernels of elementwise_table.hip take by value, finished at plan time except for pointers and scalars — immutable, shared with
    // the plan's copies — and the launch's grid
    std::shared_ptr<const EwTable> tab;
    uint32_t   tabGrid = 0;
    uint32_t   tabFromA = 0, tabFromD = 0;   // tile kernel: how many modes the tile took from A's side and from D's (the description's "tile")
    bool on_table() const { return variant == EW_TABLE_TILE || variant == EW_TABLE_GATHER; }
};
// cutensorElementwiseTrinaryExecute: D = opABC(opAB(alpha A, beta B), gamma C) as one or two passes of the
// element-wise kernels (plan_elementwise_trinary)
struct EwTrinaryPlan {
    bool   twoPass = false;      // pass 1: D = s1 * perm(X1);  last pass: D = opAC(opAB(delta * E, s2 * perm(X2)), gamma * perm(C))
    bool   swapAB = false;       // the operand that already has D's layout plays E (single pass): true -> E = B, X2 = A
    bool   bothPermuted = false; // single pass with two LDS tiles: A through the tile path, B as the second tile operand
    EwPlan first;                // permutation X1 -> D (two-pass form only)
    EwPlan last;
    // two-pass form with C overlapping D (in-place use, as elementwise_binary.cu:202-205 passes C = D): pass 1 would overwrite C before
    // the last pass reads it, so such a call runs `gather` instead — ONE launch of the element-gather kernel with A on its tile path and
    // B as X, where every lane reads its own element of C before it writes that element of D
    bool     hasGather = false;
    EwPlan   gather;
    uint64_t spanC = 0, spanD = 0;   // bytes from the first to one past the last element of C / D
};
struct ReducePlan {
    int          variant = RED_GENERIC;
    ReduceParams p{};
    uint64_t     workspace = 0;
    bool         isPermutation = false;   // no reduced modes: executed by the element-wise family
    EwPlan       perm;
    // variant RED_TABLE (a kept or reduced group of more than kMaxGroupModes digits): the mode table of reduce_table_kernel; `p` then
    // holds the totals, the split and the operators for the description, and no digits
    std::shared_ptr<const EwTable> tab;
};

// One mode of an element-wise or reduction problem while it is planned: extent and element strides per tensor
struct EwMode {
    int64_t extent;
    int64_t sA = 0, sD = 0, sC = 0;
    int64_t sX = 0;   // second permuted operand (element-wise trinary), 0 when unused
};
// Set by plan_elementwise / plan_reduction where they refuse a problem for its MODE COUNT alone ("too many unfusable modes", "mode
// group too large") — every other check passed: the fused modes they got as far as, for the mode-table route to start from.
// plan_elementwise: `modes`, sorted by D's stride; plan_reduction: `kept` and `red`, each sorted by A's stride.
struct ModeCountRefusal {
    bool hit = false;
    std::vector<EwMode> modes, kept, red;
};
// the code a kernel gets for an operand's unary operator: 0 for the operators that leave real data as it is
inline bool unary_is_plain(cutensorOperator_t o) { return o == CUTENSOR_OP_IDENTITY || o == CUTENSOR_OP_CONJ; }
inline int32_t unary_code(cutensorOperator_t o) { return unary_is_plain(o) ? 0 : (int32_t)o; }

// allowWide = false: never the tiled kernels of 8- / 16-byte elements (the trinary planner on real data: they take no E / X operand; on
// complex data its passes run on kernels of their own that do, and it allows them)
cutensorStatus_t plan_elementwise(const cutensorOperationDescriptor& op, EwPlan& plan, std::string* why, bool allowWide = true,
                                  ModeCountRefusal* over = nullptr);
cutensorStatus_t plan_elementwise_trinary(const cutensorOperationDescriptor& op, EwTrinaryPlan& plan, std::string* why);
cutensorStatus_t plan_reduction(const cutensorOperationDescriptor& op, uint64_t wsLimit, int numCUs,
                                ReducePlan& plan, std::string* why, ModeCountRefusal* over = nullptr);
// The planner of the PUBLIC permutation, binary and reduction descriptors (cutensorCreatePermutation / ElementwiseBinary / Reduction,
// cutensorEstimateWorkspaceSize, cutensorCreatePlan): plan_elementwise / plan_reduction, and exactly where those refuse a problem for
// its mode count, the mode-table route (plan_elementwise_table.cpp).  Fills `red` for a reduction descriptor, `ew` for the others.
// The planner's internal callers (trinary passes, repack, lone-mode reductions, padded permutations) keep calling the two above.
cutensorStatus_t plan_elementwise_any(const cutensorOperationDescriptor& op, uint64_t wsLimit, int numCUs, EwPlan& ew, ReducePlan& red,
                                      std::string* why);
bool ew_table_gather_forced();   // CUTENSOR_AMD_EW_TABLE=gather (hooks flavour): the gather kernel where the tile kernel applies

// ---- execute (exec_elementwise.cpp: the entry points of this family and the one path from a plan to a launch) ----------------
struct CxScalar { double re = 0.0, im = 0.0; };
inline CxScalar read_scalar(const void* s, hipDataType t) {   // a caller's alpha / beta / gamma of scalar type t (real types: im = 0)
    if (s == nullptr) return {};
    auto part = [&](int i) { return (t == HIP_R_64F || t == HIP_C_64F) ? static_cast<const double*>(s)[i] : (double)static_cast<const float*>(s)[i]; };
    return {part(0), (t == HIP_C_32F || t == HIP_C_64F) ? part(1) : 0.0};
}
inline bool misaligned(const void* p, uint32_t a) { return a > 1 && (reinterpret_cast<uintptr_t>(p) % a) != 0; }
// One launch of an element-wise plan: the operands by role, each with its scalar — A through the tile path (alpha), X the second
// permuted operand (xi), E the operand with D's strides (delta), C (gamma); a role without an operand stays null
struct EwCall {
    const void *A = nullptr, *X = nullptr, *E = nullptr, *C = nullptr;
    void*       D = nullptr;
    CxScalar    alpha, xi, delta, gamma;
};
hipError_t run_elementwise(const EwPlan& ew, hipDataType dtype, const EwCall& call, hipStream_t stream);
int describe_elementwise(const cutensorPlan& pl, char* buf, size_t len);   // ctamdDescribePlan of an element-wise or reduction plan

// Raised while the pairwise plans of a trinary or a block-sparse contraction are made or priced: under COMPUTE_DESC_32F on fp64 /
// complex128 data those keep the fp64 kernels (f64x_decide, contraction_route.cpp), and the plan memo stands aside for them
extern thread_local int t_f64xOff;
struct F64xOffScope { F64xOffScope() { ++t_f64xOff; } ~F64xOffScope() { --t_f64xOff; } };
cutensorStatus_t blocksparse_estimate(cutensorHandle_t handle, const cutensorOperationDescriptor& desc, uint64_t* ws);
cutensorStatus_t blocksparse_plan(cutensorHandle_t handle, const cutensorOperationDescriptor& desc, uint64_t wsLimit, cutensorPlan* pl);
int blocksparse_describe(const cutensorPlan& pl, char* buf, size_t len);   // ctamdDescribePlan of a block-sparse plan

FastDiv make_fastdiv(uint32_t d);
size_t  dtype_size(hipDataType t);

}  // namespace ctamd

// Incremental-autotuning trial plans are timed by cutensorContract for their first few executions only; the counter lives in
// the (otherwise immutable) plan, copyable so that plans stay copy-constructible (the plan memo clones prototypes).
struct TrialCounter {
    mutable std::atomic<int> timed{0};
    TrialCounter() = default;
    TrialCounter(const TrialCounter& o) : timed(o.timed.load(std::memory_order_relaxed)) {}
    TrialCounter& operator=(const TrialCounter& o) { timed.store(o.timed.load(std::memory_order_relaxed), std::memory_order_relaxed); return *this; }
};

// A contraction whose mode groups are too wide for the tiled kernels' argument block, peeled: the modes listed here are walked
// by the host (one launch of the inner, tiled plan per index combination, operands offset by index x stride); a contracted
// peeled mode accumulates into D, a free one writes a region of its own.
struct PeelMode {
    int64_t extent = 1;
    int64_t sA = 0, sB = 0, sC = 0, sD = 0;   // element strides of the peeled label in the user's A, B, C, D (0: not carried)
    bool    contracted = false;
};

// A plan is copyable (the plan memo clones prototypes): what it owns — sub-plans, finished and never changed after that, and the device
// copy of its mode table — is shared with its copies and released with the last of them
using SubPlan = std::shared_ptr<cutensorPlan>;

struct cutensorPlan {
    ctamd::WideParams wide{};        // mode-table contraction (PlanKind::ModeTable); .modes is filled per launch from wideDev,
    std::vector<ctamd::WideMode> wideTab;   // uploaded from this host copy at plan creation or by the first cutensorContract
    std::shared_ptr<const ctamd::WideMode> wideDev;
    // trinary contraction: the two pairwise plans, the intermediate's size and which operand plays which role
    std::shared_ptr<ctamd::BlockSparsePlan> bsp;     // block-sparse contraction: dense plans + block-pair task list
    SubPlan sub1, sub2;                              // (also: the inner plans of a peeled contraction and sub1 of a two-step one)
    std::vector<PeelMode> peel;
    // PlanKind::LoneReduce / Repack: the first step of A / B into packed temporaries at the head of the workspace (null: the operand is
    // used as it is); sub1 = the contraction
    SubPlan loneA, loneB;
    uint64_t    loneBytesA = 0, loneBytesB = 0;
    // fp16 reductions: the temporary holds sum * 2^-loneShift, loneShift = ceil(log2(n) / 2) for n summed elements, and the inner
    // contraction's alpha takes 2^(loneShiftA + loneShiftB) back (both factors exact).  Half the exponent of n, not all of it: a coherent
    // sum (n |x|) lands at sqrt(n) |x| — 65504 is reached only by inputs sqrt(n) times larger than an unscaled sum needs to overflow — and
    // a zero-mean sum (sqrt(n) |x|) stays at |x|, as precise as the inputs.  The full 2^-ceil(log2 n) would put a zero-mean temporary
    // sqrt(n) below the inputs, into the fp16 subnormals already at |x| ~ 1e-2, n ~ 1e5 (tests/test_gpu_lone_modes.py measures both)
    int         loneShiftA = 0, loneShiftB = 0;
    uint64_t    tBytes = 0;
    int         triOrder[3] = {0, 1, 2};
    OpKind      kind;
    hipDataType dtype = HIP_R_32F;
    hipDataType dtypeA = HIP_R_32F, dtypeB = HIP_R_32F;   // contractions: the caller's A and B (they differ from `dtype` in a mixed fp64 x complex128 plan)
    hipDataType scalarType = HIP_R_32F;
    uint64_t    requiredWorkspace = 0;
    uint32_t    alignA = 0, alignB = 0, alignC = 0, alignD = 0;  // pointer alignment the plan relies on
    // contraction
    ctamd::ContractionView     view;
    ctamd::ContractionChoice   choice;
    ctamd::PlanKind            planKind = ctamd::PlanKind::Simple;
    ctamd::GettParams          gett{};
    ctamd::SplitKReduceParams  skr{};
    bool                       accumulate64 = false;
    bool                       fusedFold = false;     // split-K partials are folded inside the GETT launch
    std::string                tuneKey;               // non-empty: an incremental-autotuning trial, timed by cutensorContract
    TrialCounter               trial;                 // executions of this trial plan timed so far (at most kTrialTimedRuns)
    static constexpr int       kTrialTimedRuns = 3;
    // element-wise / reduction
    ctamd::EwPlan     ew;
    ctamd::EwTrinaryPlan ew3;
    // padded permutation: the output buffer holds extents + padLeft + padRight per mode; it is filled with the
    // padding value, then the permutation writes the interior
    uint64_t          padFillElems = 0;    // 0 = no padding
    int64_t           padOffsetElems = 0;  // element offset of the interior's origin
    double            padValue = 0.0;
    uint32_t          alignB3 = 0;     // element-wise trinary: alignment of B
    ctamd::ReducePlan red;
};

struct cutensorHandle {
    int device = 0;
    bool haveDevice = false;            // a GPU was visible at cutensorCreate (false: descriptors and plans only)
    int numCUs = 256;
    std::mutex mtx;                     // syncPool / syncNext, xcdSpeed, and the late upload of a plan's mode table (mode_table_on_device)
    ctamd::PlanStore plans;             // plan cache, plan memo and incremental autotuning, behind a lock of their own (plan_store.hpp)
    // {arrivals, departures} counter pairs for in-launch split-K folds, 64 B apart, zeroed once; a launch
    // draws the next slot round-robin and its last workgroup re-arms it (gett_f32_stream.hip)
    // relative sustained shader clock of the 8 XCDs under the streaming GETT kernel (measured once per handle by
    // calibrate_xcd_split); empty = not measured, all-equal = measurement failed / disabled
    std::vector<double> xcdSpeed;
    uint32_t* syncPool = nullptr;
    uint32_t  syncNext = 0;
    static constexpr uint32_t kSyncSlots = 256;
    // diagnostics, per handle (ctamdSetSplitKFold / ctamdSetTimingBuffer / ctamdProfileBegin): a second handle — another
    // framework thread's — never sees them
    std::atomic<bool> skipFold{false};
    std::atomic<unsigned long long*> timingBuffer{nullptr};
    struct KernelProfile {
        std::atomic<bool> enabled{false};
        std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
        std::mutex mtx;
    } prof;
};

// ---- contraction routing (contraction_route.cpp) -----------------------------------------------------------------------------
namespace ctamd {

inline int log_level() {
    static int lvl = [] {
        const char* e = std::getenv("CUTENSOR_LOG_LEVEL");   // contraction_jit.cu:142 hints at this knob
        return e ? std::atoi(e) : 0;
    }();
    return lvl;
}
#define CT_LOG(...) do { if (log_level() > 0) { std::fprintf(stderr, "[cutensor-amd] " __VA_ARGS__); std::fputc('\n', stderr); } } while (0)

// pieces of the workspace start at multiples of 256 bytes
constexpr uint64_t align256(uint64_t bytes) { return (bytes + 255) & ~255ull; }
// Two-step plans (PlanKind::LoneReduce / Repack) and their estimate: A's temporary at the head of the workspace, B's at offB, the
// sub-plans' own workspace from offW on
struct TwoStepLayout {
    const uint64_t offB, offW;
    TwoStepLayout(uint64_t bytesA, uint64_t bytesB) : offB(align256(bytesA)), offW(offB + align256(bytesB)) {}
};

// the caller names a candidate of the ranked list (CUTENSOR_ALGO >= 0 or a kernel rank): it gets that candidate
inline bool names_candidate(const cutensorPlanPreference& pr) { return (int)pr.algo >= 0 || pr.kernelRank > 0; }
// ... or asks for a measured choice among the candidates (CUTENSOR_ALGO_DEFAULT_PATIENT, incremental autotuning)
inline bool names_candidate_or_tunes(const cutensorPlanPreference& pr) { return names_candidate(pr) || pr.algo == CUTENSOR_ALGO_DEFAULT_PATIENT || pr.autotune == CUTENSOR_AUTOTUNE_MODE_INCREMENTAL; }

// the kernel table a ContractionChoice::kernel of `family` indexes
const GettKernelInfo* kernel_table(int family, int* count);
// ... and the entry itself; nullptr when `kernel` is not an index into that table
const GettKernelInfo* kernel_info(int family, int kernel);

// What cutensorCreatePlan was asked for.  cutensorEstimateWorkspaceSize builds the same request for a contraction, with the cap of its
// workspace preference as the limit.
struct PlanRequest {
    cutensorHandle*                    handle;
    const cutensorOperationDescriptor& desc;
    cutensorPlanPreference_t           pref;      // as the caller passed it (may be null): what sub-plans are created with
    const cutensorPlanPreference&      pr;        // the same with the defaults filled in
    uint64_t                           wsLimit;
};
inline bool accumulates_in_fp64(const cutensorOperationDescriptor& d) { return d.compute && d.compute->id == 5; }   // COMPUTE_DESC_64F
bool plan_env_override();

// (split_lone_modes and plan_repack: the first steps — reductions or permuted copies of A / B — and the contraction on their results)
struct TwoStepSplit {
    cutensorOperationDescriptor inner, stepA, stepB;
    bool hasA = false, hasB = false;
    uint64_t bytesA = 0, bytesB = 0;       // packed sizes of the temporaries
    int64_t summedA = 1, summedB = 1;      // lone modes: elements summed into each element of a temporary
};
bool split_lone_modes(const cutensorOperationDescriptor& desc, TwoStepSplit& out);
int f64x_elem_of(const cutensorOperationDescriptor& d);
extern thread_local bool t_inRepack;
struct RepackScope { bool prev; RepackScope() : prev(t_inRepack) { t_inRepack = true; } ~RepackScope() { t_inRepack = prev; } };
// The ranked candidates of a contraction the tiled kernels can describe, and what its repack route needs to know about them
struct TiledRoute {
    bool mfmaPath = false, h16Path = false, genPath = false;   // fp32 families / aligned 16-bit family / general MFMA family (h16Path implies genPath)
    std::vector<ContractionChoice> ch;                         // best first; empty: the general family or the simple kernel
    double tDirectUs = 0.0;                                    // > 0: fp32 / fp64 / complex64 off their fast kernels — what the plan on the operands as they lie costs
    std::vector<std::string> notes;                            // the plan lines of the compute-descriptor decisions, for the builder to log
    int family() const { return mfmaPath ? 0 : h16Path ? 1 : 2; }
};
// the routes in the order they are tried (contraction_route.cpp); each says whether it applies and returns what the builder and the
// estimate need
bool route_peeled(const PlanRequest& rq, const ContractionView& v, cutensorOperationDescriptor& inner, std::vector<PeelMode>& peel);
bool route_mode_table(const PlanRequest& rq, ContractionView& v, bool accumulate64);
TiledRoute rank_tiled_candidates(const PlanRequest& rq, const ContractionView& v, bool accumulate64);
bool route_repack(const PlanRequest& rq, const ContractionView& v, const TiledRoute& r, TwoStepSplit& rs);
void route_tiled(const PlanRequest& rq, const ContractionView& v, TiledRoute& r);
cutensorStatus_t estimate_contraction(const PlanRequest& rq, cutensorWorksizePreference_t workspacePref, uint64_t* estimate);

// ---- the two helpers plan creation (create_plan.cpp) and execution (exec_contraction.cpp) share ---------------------------------
// the fold that matches a kernel's split-K partials (exec_contraction.cpp; the measured selection of create_plan.cpp times it too)
CTAMD_HIDDEN hipError_t launch_splitk_fold(int family, const GettKernelInfo& k, const SplitKReduceParams& r, hipStream_t stream);
// the mode table of a plan in device memory; null: no memory, or no device (create_plan.cpp; exec_contraction.cpp uploads late)
CTAMD_HIDDEN std::shared_ptr<const WideMode> upload_mode_table(const std::vector<WideMode>& tab);

}  // namespace ctamd
