// exec_contraction.cpp — cutensorContract and cutensorContractTrinary: the path from a contraction plan to its launches (two-step and
// peeled plans as calls of their inner plans; the mode-table, tiled and simple kernels with the split-K fold), the launch counters, and
// the diagnostics that read or set what this file owns.  Each entry point cites the reference call site it serves.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

#include "internal.hpp"

using namespace ctamd;

namespace {

// launches of cutensorContract by kernel kind since the library was loaded (ctamdLaunchCounts): 0 = gett_simple_kernel (scalar FMA
// fallback), 1 = gett_wide_kernel (mode table), 2 = fp32 MFMA families, 3 = aligned 16-bit MFMA family, 4 = general MFMA family
std::atomic<uint64_t> g_launchCounts[5];
std::atomic<int> g_lastH16Kernel{-1};   // table entry of the last launch of the aligned 16-bit family (ctamdLastH16Kernel: which twin ran)

}  // namespace

// the fold that matches a kernel's split-K partials: accumulator-register order (fp32 ring kernels), row-major fp32, or — general family
// with 8- / 16-byte elements — row-major partials in the accumulator type
hipError_t ctamd::launch_splitk_fold(int family, const GettKernelInfo& k, const SplitKReduceParams& r, hipStream_t stream) {
    // (the mixed fp64 x complex128 kernels write complex128's double2 partials: complex128's fold takes them as they are)
    if (family == 2 && !gen_elem_f32_partials(k.elem)) return launch_gen_splitk_reduce(r, k.elem == GEN_RC64 ? (int)GEN_C64 : k.elem, stream);
    return k.fragPartials ? launch_splitk_reduce_frag(r, stream) : launch_splitk_reduce(r, stream);
}

// alpha and beta of a call as the kernels take them, and 1 / 0 in a plan's scalar type ({re, im} pairs: also the complex ones)
struct CallScalars { double a, b, aIm, bIm; };
static const void* scalar_constant(hipDataType scalarType, bool one) {
    static const float f[2][2] = {{0.f, 0.f}, {1.f, 0.f}};
    static const double d[2][2] = {{0.0, 0.0}, {1.0, 0.0}};
    return (scalarType == HIP_R_64F || scalarType == HIP_C_64F) ? static_cast<const void*>(d[one]) : static_cast<const void*>(f[one]);
}
// LoneReduce / Repack plans: the first step of an operand is a reduction over its lone modes (split_lone_modes) or a permuted copy
// (plan_repack) into its packed temporary at the head of the workspace; then the inner contraction runs on the temporaries
static cutensorStatus_t run_two_step(const cutensorHandle_t handle, const cutensorPlan& plan, const void* alpha, const void* A, const void* B,
                                     const void* beta, const void* C, void* D, void* workspace, uint64_t workspaceSize, cudaStream_t stream) {
    if (!plan.sub1) return CUTENSOR_STATUS_INVALID_VALUE;
    const TwoStepLayout lay(plan.loneBytesA, plan.loneBytesB);
    char* ws = static_cast<char*>(workspace);
    const void* one = scalar_constant(plan.scalarType, true);
    const void* zero = scalar_constant(plan.scalarType, false);
    // fp16 temporaries (float scalars): scaled down by exact powers of two, alpha scaled up by their product (loneShiftA: internal.hpp)
    const float scaleA = std::ldexp(1.f, -plan.loneShiftA), scaleB = std::ldexp(1.f, -plan.loneShiftB);
    const bool scaled = plan.loneShiftA + plan.loneShiftB > 0;
    const float alphaScaled = scaled ? *static_cast<const float*>(alpha) * std::ldexp(1.f, plan.loneShiftA + plan.loneShiftB) : 0.f;
    auto first_step = [&](const SubPlan& step, const float& scale, const void* X, char* T) {
        return plan.planKind == PlanKind::Repack ? cutensorPermute(handle, step.get(), one, X, T, stream)
                                                 : cutensorReduce(handle, step.get(), scaled ? &scale : one, X, zero, T, T, ws + lay.offW, workspaceSize - lay.offW, stream);
    };
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    if (plan.loneA) { st = first_step(plan.loneA, scaleA, A, ws); A = ws; }
    if (st == CUTENSOR_STATUS_SUCCESS && plan.loneB) { st = first_step(plan.loneB, scaleB, B, ws + lay.offB); B = ws + lay.offB; }
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    return cutensorContract(handle, plan.sub1.get(), scaled ? &alphaScaled : alpha, A, B, beta, C, D, ws + lay.offW, workspaceSize - lay.offW, stream);
}
// Peeled plans: every index combination of the peeled modes is one launch of the inner plan on offset operands; a combination whose
// contracted indices are all zero writes its region of D first (caller's beta, caller's C), the others accumulate into it
static cutensorStatus_t run_peeled(const cutensorHandle_t handle, const cutensorPlan& plan, const void* alpha, const void* A, const void* B,
                                   const void* beta, const void* C, void* D, void* workspace, uint64_t workspaceSize, cudaStream_t stream) {
    if (!plan.sub1) return CUTENSOR_STATUS_INVALID_VALUE;
    const int64_t es = (int64_t)dtype_size(plan.dtype);      // C and D; A and B at their own element size (a mixed plan's real input: 8 bytes)
    const int64_t esA = (int64_t)dtype_size(plan.dtypeA), esB = (int64_t)dtype_size(plan.dtypeB);
    const void* one = scalar_constant(plan.scalarType, true);
    const size_t n = plan.peel.size();
    std::vector<int64_t> digit(n, 0);
    for (;;) {
        int64_t oA = 0, oB = 0, oC = 0, oD = 0;
        bool first = true;
        for (size_t i = 0; i < n; ++i) {
            const PeelMode& pm = plan.peel[i];
            oA += digit[i] * pm.sA; oB += digit[i] * pm.sB; oC += digit[i] * pm.sC; oD += digit[i] * pm.sD;
            if (pm.contracted && digit[i] != 0) first = false;
        }
        char* d = static_cast<char*>(D) + oD * es;
        const char* c = first ? (C ? static_cast<const char*>(C) + oC * es : nullptr) : d;
        // accumulate launches read D in D's own layout (sub2, when the caller's C is laid out differently or conjugated)
        const cutensorStatus_t st = cutensorContract(handle, (!first && plan.sub2) ? plan.sub2.get() : plan.sub1.get(), alpha, static_cast<const char*>(A) + oA * esA,
                                                     static_cast<const char*>(B) + oB * esB, first ? beta : one, c, d, workspace, workspaceSize, stream);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        size_t i = 0;
        for (; i < n; ++i) {
            if (++digit[i] < plan.peel[i].extent) break;
            digit[i] = 0;
        }
        if (i == n) return CUTENSOR_STATUS_SUCCESS;
    }
}
// Per-kernel timing (ctamdProfileBegin): an event pair around the GETT launch of a tiled plan, kept by the handle
struct ProfiledLaunch {
    cutensorHandle* handle;
    hipStream_t stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ProfiledLaunch(cutensorHandle* h, hipStream_t s) : handle(h), stream(s) {
        if (h->prof.enabled.load(std::memory_order_relaxed) && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess)
            (void)hipEventRecord(e0, stream);
    }
    void end() {
        if (!e0 || !e1) return;
        (void)hipEventRecord(e1, stream);
        std::lock_guard<std::mutex> g(handle->prof.mtx);
        handle->prof.events.emplace_back(e0, e1);
    }
};
static bool mode_table_on_device(const cutensorHandle_t handle, cutensorPlan& plan) {
    if (plan.wideDev) return true;
    std::lock_guard<std::mutex> g(handle->mtx);
    if (!plan.wideDev) plan.wideDev = upload_mode_table(plan.wideTab);
    return plan.wideDev != nullptr;
}
static hipError_t launch_mode_table(const cutensorPlan& plan, const GettParams& p, const CallScalars& s, hipStream_t stream) {
    WideParams w = plan.wide;
    w.modes = plan.wideDev.get();
    w.A = p.A; w.B = p.B; w.C = p.C; w.D = p.D;
    w.alpha = p.alpha; w.beta = p.beta; w.alpha64 = s.a; w.beta64 = s.b;
    w.alphaIm = s.aIm; w.betaIm = s.bIm;
    g_launchCounts[1].fetch_add(1, std::memory_order_relaxed);
    return launch_gett_wide(w, (int)plan.dtype, plan.accumulate64, stream);
}
// Strip plan (ContractionChoice::stripKernel): the interior's whole tiles on kernel `ki`, then the two edge strips (rows past mInt x all
// columns, rows below mInt x columns past nInt) as ONE launch of the 64 x 64 tile `ks` with two tile rectangles
static hipError_t launch_strip_plan(const ContractionChoice& c, const GettKernelInfo& ki, const GettKernelInfo& ks, const GettParams& p, hipStream_t stream) {
    const uint32_t mInt = c.mInt, nInt = c.nInt, Mt = p.gM.total, Nt = p.gN.total, Lt = p.gL.total;
    GettParams q = p;
    q.tilesM = mInt / (uint32_t)ki.bm; q.tilesN = nInt / (uint32_t)ki.bn;
    q.nBlocks = q.tilesM * q.tilesN * Lt;
    const hipError_t err = ki.launch(q, stream);
    GettParams s2 = p;
    s2.mOrg = mInt; s2.nOrg = 0;
    s2.tilesM = (Mt - mInt + (uint32_t)ks.bm - 1u) / (uint32_t)ks.bm; s2.tilesN = (Nt + (uint32_t)ks.bn - 1u) / (uint32_t)ks.bn;
    s2.mOrg2 = 0; s2.nOrg2 = nInt;
    s2.tilesM2 = (mInt + (uint32_t)ks.bm - 1u) / (uint32_t)ks.bm; s2.tilesN2 = (Nt - nInt + (uint32_t)ks.bn - 1u) / (uint32_t)ks.bn;
    if (s2.tilesM * s2.tilesN == 0u) {     // no rows past the interior: the column strip is the only rectangle
        s2.mOrg = s2.mOrg2; s2.nOrg = s2.nOrg2; s2.tilesM = s2.tilesM2; s2.tilesN = s2.tilesN2;
        s2.tilesM2 = s2.tilesN2 = 0;
    }
    s2.nBlocks = (s2.tilesM * s2.tilesN + s2.tilesM2 * s2.tilesN2) * Lt;
    return (err == hipSuccess && s2.nBlocks > 0u) ? ks.launch(s2, stream) : err;
}
// Tiled plans: the GETT launch of the plan's kernel and, for split-K, the fold that matches the kernel's partials
static hipError_t launch_tiled(const cutensorHandle_t handle, const cutensorPlan& plan, GettParams& p, const CallScalars& s, void* workspace, hipStream_t stream) {
    const ContractionChoice& c = plan.choice;
    int count = 0;
    const GettKernelInfo* tab = kernel_table(c.family, &count);
    g_launchCounts[2 + c.family].fetch_add(1, std::memory_order_relaxed);
    p.partial = (c.splitK > 1) ? static_cast<float*>(workspace) : nullptr;
    int launchKernel = c.kernel;
    if (c.family == 0) {
        static const int policy = [] { const char* e = CTAMD_HOOK_ENV("CUTENSOR_AMD_PARTIAL_STORE"); return e ? (e[0] == 'p' ? 1 : e[0] == 'n' ? 2 : e[0] == 's' ? 3 : 0) : 0; }();   // hooks flavour; 's': the row epilogue skips its stores (timing only)
        p.partialPolicy = policy;
        {   // hooks flavour, read per call: a test runs every entry in one process
            const char* e = CTAMD_HOOK_ENV("CUTENSOR_AMD_FLAT_START");
            p.noFlatStart = (e == nullptr) ? FLAT_START_ARGS : e[0] == '0' ? FLAT_START_GENERAL : e[0] == '2' ? FLAT_START_STRUCT
                            : e[0] == '3' ? FLAT_START_ARGS_FOLD : e[0] == '4' ? FLAT_START_ARGS_GETT : FLAT_START_ARGS;
        }
        if (plan.fusedFold) {
            uint32_t slot;
            {
                std::lock_guard<std::mutex> g(handle->mtx);
                slot = handle->syncNext++ % cutensorHandle::kSyncSlots;
            }
            p.sync = handle->syncPool + (size_t)slot * 16;
        }
    } else if (c.family == 1) {
        // beta is known only now.  The persistent 16-bit kernel (H16_W4P) streams its tiles with beta != 0 too since round 6 (C joins the
        // accumulators through the idle row image: gett_h16p.hip) — when C has the 16-byte lanes of D (its fastest N mode contiguous).
        // Any other C sends every tile through the ring-resident epilogue, where the kernel is slower than its one-tile twin (H16_W4X:
        // same tile, same arguments, same workspace; profiles/r05r_h16p_beta.jsonl): the twin is launched then
        // (CUTENSOR_AMD_H16_WAVES=4p names the kernel for every call: the tests of that path)
        static const bool persistentForced = CTAMD_HOOK_ENV("CUTENSOR_AMD_H16_WAVES") != nullptr && h16_waves_variant() == H16_W4P;
        if (tab[launchKernel].variant == H16_W4P && s.b != 0.0 && p.cStrideN[0] != 1 && !persistentForced)
            launchKernel = h16_entry(H16_W4X, launchKernel - H16_W4P);
        g_lastH16Kernel.store(launchKernel, std::memory_order_relaxed);
    }
    ProfiledLaunch prof(handle, stream);
    hipError_t err = (c.family == 1 && c.stripKernel >= 0 && c.stripKernel < count) ? launch_strip_plan(c, tab[launchKernel], tab[c.stripKernel], p, stream)
                                                                                    : tab[launchKernel].launch(p, stream);
    prof.end();
    if (err != hipSuccess || c.splitK <= 1 || (c.family == 0 && (plan.fusedFold || handle->skipFold.load(std::memory_order_relaxed)))) return err;
    SplitKReduceParams r = plan.skr;
    r.partial = static_cast<float*>(workspace);
    r.C = p.C; r.D = p.D; r.alpha = p.alpha; r.beta = p.beta;
    r.alpha64 = s.a; r.beta64 = s.b; r.alphaIm = s.aIm; r.betaIm = s.bIm; r.conjC = p.conjC;
    r.noFlatStart = p.noFlatStart;
    return launch_splitk_fold(c.family, tab[c.kernel], r, stream);
}

extern "C" {

// contraction.cu:261-265, einsum.cu:334-338
cutensorStatus_t cutensorContract(const cutensorHandle_t handle, const cutensorPlan_t plan, const void* alpha,
                                  const void* A, const void* B, const void* beta, const void* C, void* D,
                                  void* workspace, uint64_t workspaceSize, cudaStream_t stream) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || plan->kind != OpKind::Contraction) return CUTENSOR_STATUS_INVALID_VALUE;
    if (alpha == nullptr || beta == nullptr || A == nullptr || B == nullptr || D == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    const CxScalar ca = read_scalar(alpha, plan->scalarType), cb = read_scalar(beta, plan->scalarType);
    const CallScalars s{ca.re, cb.re, ca.im, cb.im};
    const bool betaZero = (s.b == 0.0 && s.bIm == 0.0);
    if (!betaZero && C == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (misaligned(A, plan->alignA) || misaligned(B, plan->alignB) || misaligned(D, plan->alignD) ||
        (!betaZero && misaligned(C, plan->alignC)))
        return CUTENSOR_STATUS_INVALID_VALUE;
    if (plan->requiredWorkspace > 0 && (workspace == nullptr || workspaceSize < plan->requiredWorkspace))
        return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
    switch (plan->planKind) {
        case PlanKind::LoneReduce:
        case PlanKind::Repack: return run_two_step(handle, *plan, alpha, A, B, beta, C, D, workspace, workspaceSize, stream);
        case PlanKind::Peeled: return run_peeled(handle, *plan, alpha, A, B, beta, C, D, workspace, workspaceSize, stream);
        case PlanKind::ModeTable:   // first execution of a plan made without a device: the mode table moves there (kept until the plan dies)
            if (!mode_table_on_device(handle, *plan)) return CUTENSOR_STATUS_ALLOC_FAILED;
            break;
        default: break;
    }
    GettParams p = plan->gett;
    p.A = plan->view.swapped ? B : A;
    p.B = plan->view.swapped ? A : B;
    p.C = (!betaZero) ? C : D;
    p.D = D;
    p.alpha = (float)s.a; p.beta = (float)s.b;
    p.alpha64 = s.a; p.beta64 = s.b;
    p.alphaIm = s.aIm; p.betaIm = s.bIm;
    p.endA += (unsigned long long)(uintptr_t)p.A;   // the plan holds the operands' byte spans (fill_gett_params)
    p.endB += (unsigned long long)(uintptr_t)p.B;
    p.timing = handle->timingBuffer.load(std::memory_order_relaxed);
    // incremental-autotuning trial: one event pair around everything this call launches, read later (PlanStore::resolve)
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // only the first kTrialTimedRuns executions of a trial plan are timed: a plan created once and run in a loop neither
    // grows the pending list nor pays event creation per launch
    if (!plan->tuneKey.empty() && plan->trial.timed.load(std::memory_order_relaxed) < cutensorPlan::kTrialTimedRuns &&
        plan->trial.timed.fetch_add(1, std::memory_order_relaxed) < cutensorPlan::kTrialTimedRuns) {
        if (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess) {
            (void)hipGetLastError();
            if (t0) (void)hipEventDestroy(t0);
            t0 = t1 = nullptr;
        } else {
            (void)hipEventRecord(t0, stream);
        }
    }
    hipError_t err;
    if (plan->planKind == PlanKind::ModeTable) err = launch_mode_table(*plan, p, s, stream);
    else if (plan->planKind == PlanKind::Tiled) err = launch_tiled(handle, *plan, p, s, workspace, stream);
    else {
        g_launchCounts[0].fetch_add(1, std::memory_order_relaxed);
        p.partial = nullptr;
        err = launch_gett_simple(p, (int)plan->dtype, plan->accumulate64, stream);
    }
    if (t0 != nullptr) {
        if (err == hipSuccess && hipEventRecord(t1, stream) == hipSuccess) {
            handle->plans.add_measurement(plan->tuneKey, plan->choice.kernel, plan->choice.splitK, t0, t1);
        } else {   // a failed launch is not a measurement
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
        }
    }
    if (err != hipSuccess) { CT_LOG("cutensorContract: %s", hipGetErrorString(err)); return CUTENSOR_STATUS_EXECUTION_FAILED; }
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_trinary.cu:290-294
cutensorStatus_t cutensorContractTrinary(const cutensorHandle_t handle, const cutensorPlan_t plan, const void* alpha,
                                         const void* A, const void* B, const void* C, const void* beta, const void* D, void* E,
                                         void* workspace, uint64_t workspaceSize, cudaStream_t stream) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || plan->kind != OpKind::ContractionTrinary || !plan->sub1 || !plan->sub2) return CUTENSOR_STATUS_INVALID_VALUE;
    if (alpha == nullptr || beta == nullptr || A == nullptr || B == nullptr || C == nullptr || E == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (workspace == nullptr || workspaceSize < plan->requiredWorkspace) return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
    if (misaligned(workspace, 128)) return CUTENSOR_STATUS_INVALID_VALUE;   // the intermediate and the sub-plans ask for 128 (contraction.cu:242 asserts no more)
    const void* in[3] = {A, B, C};
    const void *X = in[plan->triOrder[0]], *Y = in[plan->triOrder[1]], *Z = in[plan->triOrder[2]];
    const uint64_t tOff = align256(plan->tBytes);
    void* T = workspace;
    void* ws = static_cast<char*>(workspace) + tOff;
    const void *one = scalar_constant(plan->scalarType, true), *zero = scalar_constant(plan->scalarType, false);
    cutensorStatus_t st = cutensorContract(handle, plan->sub1.get(), one, X, Y, zero, T, T, ws, workspaceSize - tOff, stream);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    return cutensorContract(handle, plan->sub2.get(), alpha, T, Z, beta, D, E, ws, workspaceSize - tOff, stream);
} CTAMD_API_CATCH

// cutensorContract launches by kernel kind since the library was loaded: out[0] gett_simple_kernel (scalar FMA fallback), [1]
// gett_wide_kernel (mode table), [2] fp32 MFMA families, [3] aligned 16-bit MFMA family, [4] general MFMA family.  Lets a test that
// drives the library through someone else's binding (the reference's own einsum.cc) assert which kernels its cases ran on.
void ctamdLaunchCounts(uint64_t out[5]) try {
    for (int i = 0; i < 5; ++i) out[i] = g_launchCounts[i].load(std::memory_order_relaxed);
} CTAMD_API_CATCH_VOID
int ctamdLastH16Kernel(void) try { return g_lastH16Kernel.load(std::memory_order_relaxed); } CTAMD_API_CATCH_INT

// Launches of the fp32 ring kernels that took the flat entry (kernels/gett_f32_stream.hip, launch_stream) since the library was loaded:
// tells a test which of the two entries its case ran on.
uint64_t ctamdFlatStartCount(void) try { return g_flatStartLaunches.load(std::memory_order_relaxed); } CTAMD_API_CATCH_ZERO

// Diagnostics, all per handle.  Device buffer of 8 x uint64 per workgroup that the GETT kernel fills with phase
// timestamps (shader clock and wall clock); nullptr switches it off.
void ctamdSetTimingBuffer(cutensorHandle_t handle, void* deviceBuffer) try {
    if (handle != nullptr) handle->timingBuffer.store(static_cast<unsigned long long*>(deviceBuffer), std::memory_order_relaxed);
} CTAMD_API_CATCH_VOID

// enabled = 0 makes cutensorContract on this handle launch the GETT kernel only (the split-K partials stay unfolded, D is
// not written) so that a stream of back-to-back GETT launches can be timed with one event pair — per-launch event
// pairs put a ~6 us idle gap after every kernel and the chip leaves its steady clock state.  Never used by the samples.
void ctamdSetSplitKFold(cutensorHandle_t handle, int enabled) try {
    if (handle != nullptr) handle->skipFold.store(enabled == 0, std::memory_order_relaxed);
} CTAMD_API_CATCH_VOID

// Per-kernel timing of the GETT kernel inside cutensorContract on this handle: Begin() arms it, End() synchronises the
// recorded event pairs and returns the number of launches and their mean / min duration in ms.
void ctamdProfileBegin(cutensorHandle_t handle) try {
    if (handle == nullptr) return;
    std::lock_guard<std::mutex> g(handle->prof.mtx);
    handle->prof.events.clear();
    handle->prof.enabled.store(true, std::memory_order_relaxed);
} CTAMD_API_CATCH_VOID
int ctamdProfileEnd(cutensorHandle_t handle, float* meanMs, float* minMs) try {
    if (handle == nullptr) return 0;
    std::lock_guard<std::mutex> g(handle->prof.mtx);
    handle->prof.enabled.store(false, std::memory_order_relaxed);
    double sum = 0.0;
    float mn = 1e30f;
    int n = 0;
    for (auto& ev : handle->prof.events) {
        float t = 0.f;
        if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) {
            sum += t;
            mn = std::min(mn, t);
            ++n;
        }
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    handle->prof.events.clear();
    if (meanMs) *meanMs = n ? (float)(sum / n) : 0.f;
    if (minMs) *minMs = n ? mn : 0.f;
    return n;
} CTAMD_API_CATCH_INT

}  // extern "C"
