// describe.cpp — diagnostics that read a plan or the kernel tables (not part of the cuTENSOR ABI; used by the tests, the tools and the
// bench): ctamdDescribePlan for contraction plans (element-wise and reduction plans: exec_elementwise.cpp, block-sparse ones:
// blocksparse.cpp), what cuTENSORMg asks about a plan, and the counts of kernels and candidates.
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "internal.hpp"

using namespace ctamd;

extern "C" {

// A contraction plan that fell to the mode-table kernel because a group has more unfusable modes than the tiled kernels'
// argument block describes: its canonical modes as (group 0 = L, 1 = M, 2 = N, 3 = K; caller's label; extent), at most maxOut of
// them; returns how many there are, 0 for every other plan.  cuTENSORMg uses it to peel one digit of an oversized group into a
// host loop (mg/mg_contraction_plan.cpp) instead of running the functional kernel.
int ctamdPlanModeTableGroups(const cutensorPlan_t plan, int32_t* group, int32_t* label, int64_t* extent, int maxOut) try {
    if (plan == nullptr || plan->kind != OpKind::Contraction || plan->planKind != PlanKind::ModeTable) return 0;
    if (plan->view.dtype == HIP_C_32F || plan->view.dtype == HIP_C_64F) return 0;     // complex data: not a matter of mode counts
    int n = 0;
    const std::vector<CanonMode>* gs[4] = {&plan->view.L, &plan->view.M, &plan->view.N, &plan->view.K};
    bool oversized = false;
    for (int g = 0; g < 4; ++g) oversized = oversized || (int)gs[g]->size() > kMaxGroupModes;
    if (!oversized) return 0;                                                          // wide for another reason (>= 2^31 elements)
    for (int g = 0; g < 4; ++g)
        for (const CanonMode& m : *gs[g]) {
            if (n < maxOut) { if (group) group[n] = g; if (label) label[n] = m.label; if (extent) extent[n] = m.extent; }
            ++n;
        }
    return n;
} CTAMD_API_CATCH_INT

// Launches of the inner plan a peeled contraction plan makes per call (peel_wide_contraction); 0 for every other plan.
int ctamdPlanPeelLaunches(const cutensorPlan_t plan) try {
    if (plan == nullptr || plan->kind != OpKind::Contraction || plan->planKind != PlanKind::Peeled) return 0;
    long long n = 1;
    for (const PeelMode& pm : plan->peel) n *= pm.extent;
    return (int)n;
} CTAMD_API_CATCH_INT

// buf holds n characters of a plan's own keys, `{"key":..,"key":..,` — the keys of its inner plan follow: the inner plan's description is
// written over the trailing ',' and its '{' turned into that ','
static int describe_inner(const cutensorPlan& plan, char* buf, size_t len, int n);
// Writes a one-line JSON description of the plan's kernel choice into buf.
int ctamdDescribePlan(const cutensorPlan_t plan, char* buf, size_t len) try {
    if (plan == nullptr || buf == nullptr || len == 0) return -1;
    int n = 0;
    if (plan->kind == OpKind::BlockSparseContraction) return blocksparse_describe(*plan, buf, len);
    if (plan->kind == OpKind::ContractionTrinary) {
        // "order": the inputs (0 = A, 1 = B, 2 = C) as the two steps take them — X and Y contracted first, then Z; the two pairwise plans' own descriptions
        n = std::snprintf(buf, len, "{\"op\":\"contraction_trinary\",\"intermediate_bytes\":%llu,\"workspace\":%llu,\"order\":[%d,%d,%d]",
                          (unsigned long long)plan->tBytes, (unsigned long long)plan->requiredWorkspace, plan->triOrder[0], plan->triOrder[1], plan->triOrder[2]);
        for (int i = 0; i < 2; ++i) {
            if (n < 0 || (size_t)n >= len) return -1;
            n += std::snprintf(buf + n, len - (size_t)n, ",\"step%d\":", i + 1);
            if ((size_t)n >= len) return -1;
            const cutensorPlan_t step = i == 0 ? plan->sub1.get() : plan->sub2.get();
            const int m = step ? ctamdDescribePlan(step, buf + n, len - (size_t)n) : -1;
            if (m < 0 || (size_t)(n + m) >= len) return -1;
            n += m;
        }
        return n + std::snprintf(buf + n, len - (size_t)n, "}");
    }
    if (plan->kind == OpKind::Contraction && plan->planKind == PlanKind::Peeled && plan->sub1) {
        // peeled contraction: the inner (tiled) plan's description with the peel in front (and how many peeled modes are contracted ones)
        long long launches = 1;
        int contracted = 0;
        for (const PeelMode& pm : plan->peel) { launches *= pm.extent; contracted += pm.contracted ? 1 : 0; }
        n = std::snprintf(buf, len, "{\"peeled_modes\":%zu,\"peeled_contracted\":%d,\"peel_launches\":%lld,", plan->peel.size(), contracted, launches);
        return describe_inner(*plan, buf, len, n);
    }
    if (plan->kind == OpKind::Contraction && (plan->planKind == PlanKind::LoneReduce || plan->planKind == PlanKind::Repack) && plan->sub1) {
        // a two-step plan: which operands are reduced over their lone modes / copied into packed temporaries first, then the inner contraction's description
        const bool rep = plan->planKind == PlanKind::Repack, hasA = (bool)plan->loneA, hasB = (bool)plan->loneB;
        n = std::snprintf(buf, len, "{\"lone_reduce_A\":%d,\"lone_reduce_B\":%d,\"repack_A\":%d,\"repack_B\":%d,\"lone_bytes\":%llu,",
                          (hasA && !rep) ? 1 : 0, (hasB && !rep) ? 1 : 0, (hasA && rep) ? 1 : 0, (hasB && rep) ? 1 : 0,
                          (unsigned long long)(plan->loneBytesA + plan->loneBytesB));
        return describe_inner(*plan, buf, len, n);
    }
    if (plan->kind == OpKind::Contraction) {
        // "kernel": the table index of a tiled plan, else the code tools know the plan kinds by
        static const int kindCode[] = {0, -1, -2, -3, -4, -4};   // PlanKind::Tiled (unused), Simple, ModeTable, Peeled, LoneReduce, Repack
        int count = 0;
        const GettKernelInfo* tab = kernel_table(plan->choice.family, &count);
        const int k = plan->planKind == PlanKind::Tiled ? plan->choice.kernel : -1;
        n = std::snprintf(buf, len,
                          "{\"op\":\"contraction\",\"family\":%d,\"L\":%llu,\"M\":%llu,\"N\":%llu,\"K\":%llu,\"swapped\":%d,\"layA\":%d,\"layB\":%d,"
                          "\"kernel\":%d,\"bm\":%d,\"bn\":%d,\"bk\":%d,\"wm\":%d,\"wn\":%d,\"wk\":%d,\"pf\":%d,\"abl\":%d,\"splitK\":%u,\"kPerSlice\":%u,"
                          "\"blocks\":%u,\"workspace\":%llu,\"model_us\":%.2f,\"fusedFold\":%d,\"xcdTiles\":\"%016llx\",\"kname\":\"%s\"",
                          plan->choice.family, (unsigned long long)plan->view.totL, (unsigned long long)plan->view.totM,
                          (unsigned long long)plan->view.totN, (unsigned long long)plan->view.totK, (int)plan->view.swapped,
                          plan->view.layA, plan->view.layB, k >= 0 ? k : kindCode[(int)plan->planKind], k >= 0 ? tab[k].bm : 16, k >= 0 ? tab[k].bn : 16,
                          k >= 0 ? tab[k].bk : 16, k >= 0 ? tab[k].wm : 1, k >= 0 ? tab[k].wn : 1, k >= 0 ? tab[k].wk : 1,
                          k >= 0 ? tab[k].pf : 0, k >= 0 ? tab[k].ablation : 0,
                          plan->gett.splitK, plan->gett.kPerSlice, plan->gett.nBlocks,
                          (unsigned long long)plan->requiredWorkspace, plan->choice.estimateUs, (int)plan->fusedFold,
                          (unsigned long long)plan->gett.xcdTiles,
                          k >= 0 ? tab[k].name : plan->planKind == PlanKind::ModeTable ? "gett_wide_kernel" : "gett_simple_kernel");
        // contracted digits, fastest first: [extent, strideA, strideB]
        if (n > 0 && (size_t)n < len && k >= 0)     // 1: the kernel streams its operands with the nontemporal policy (no Infinity-Cache allocation)
            n += std::snprintf(buf + n, len - n, ",\"nt\":%d", tab[k].nt);
        if (n > 0 && (size_t)n < len && plan->choice.family == 2 && k >= 0)
            n += std::snprintf(buf + n, len - n, ",\"orientA\":%d,\"orientB\":%d,\"vec\":%d,\"elem\":%d", tab[k].layA, tab[k].layB, tab[k].vec, tab[k].elem);
        // a mixed fp64 x complex128 plan: which of the CALLER's inputs is the real one (0 = A, 1 = B); "vec" above is that operand's width
        if (n > 0 && (size_t)n < len && plan->view.realSide >= 0) n += std::snprintf(buf + n, len - n, ",\"real\":%d", plan->view.real_input());
        // 16-bit family: whether the launch is the RAG instantiation (masked / repaired last K-tile), and the strip plan — interior
        // [0, mInt) x [0, nInt) on `kernel`, the two edge strips as one launch of the 64 x 64 tile (ContractionChoice::stripKernel)
        if (n > 0 && (size_t)n < len && plan->choice.family == 1 && k >= 0)
            n += std::snprintf(buf + n, len - n, ",\"rag\":%d,\"strips\":%d,\"mInt\":%u,\"nInt\":%u",
                               (plan->gett.gK.total % 64u != 0u || (plan->gett.ragged & 1u)) ? 1 : 0, plan->choice.stripKernel >= 0 ? 1 : 0,
                               plan->choice.mInt, plan->choice.nInt);
        if (n > 0 && (size_t)n < len) n += std::snprintf(buf + n, len - n, ",\"Kdigits\":[");
        for (size_t i = 0; i < plan->view.K.size() && n > 0 && (size_t)n < len; ++i)
            n += std::snprintf(buf + n, len - n, "%s[%lld,%lld,%lld]", i ? "," : "", (long long)plan->view.K[i].extent,
                               (long long)plan->view.K[i].sA, (long long)plan->view.K[i].sB);
        if (n > 0 && (size_t)n < len) n += std::snprintf(buf + n, len - n, "]}");
    } else {
        n = describe_elementwise(*plan, buf, len);   // element-wise and reduction plans (exec_elementwise.cpp)
    }
    return n;
} CTAMD_API_CATCH_INT
static int describe_inner(const cutensorPlan& plan, char* buf, size_t len, int n) {
    if (n < 0 || (size_t)n >= len) return -1;
    const int m = ctamdDescribePlan(plan.sub1.get(), buf + n - 1, len - (size_t)n + 1);
    if (m < 0) return -1;
    buf[n - 1] = ',';
    return n - 1 + m;
}

// The mode table of an element-wise or reduction plan on the kernels of elementwise_table.hip, byte for byte as a launch passes it
// (pointers and scalars zero): what tests/harness/ew_table_layout_harness.cpp walks on the CPU.  Returns sizeof(EwTable), 0 for a plan
// that has none, -1 for a buffer too small.
int ctamdEwTable(const cutensorPlan_t plan, void* buf, size_t len) try {
    if (plan == nullptr || buf == nullptr) return -1;
    const EwTable* tab = nullptr;
    if (plan->kind == OpKind::Reduction) tab = plan->red.isPermutation ? plan->red.perm.tab.get() : plan->red.tab.get();
    else if (plan->kind == OpKind::Permutation || plan->kind == OpKind::ElementwiseBinary) tab = plan->ew.tab.get();
    if (tab == nullptr) return 0;
    if (len < sizeof(EwTable)) return -1;
    std::memcpy(buf, tab, sizeof(EwTable));
    return (int)sizeof(EwTable);
} CTAMD_API_CATCH_INT

// 1 when this library reads the test / measurement switches (CTAMD_HOOK_ENV: the lib_hooks/ flavour)
int ctamdTestHooksBuilt(void) try { return CTAMD_HOOKS_BUILT; } CTAMD_API_CATCH_INT

// CUTENSOR_LOG_LEVEL as this library read it: libcutensorMg.so logs its refusals under the same switch without reading it itself
int ctamdLogLevel(void) try { return log_level(); } CTAMD_API_CATCH_INT

// Instantiated fp32 GETT kernels (test coverage bookkeeping): table size, and whether entry i is a
// measurement-only ablation variant (never planned unless CUTENSOR_AMD_ABLATION is set).
int ctamdKernelCount(void) try {
    int count = 0;
    (void)kernel_table(0, &count);
    return count;
} CTAMD_API_CATCH_INT
int ctamdKernelIsAblation(int i) try {
    const GettKernelInfo* k = kernel_info(0, i);
    return (k != nullptr && k->ablation) ? 1 : 0;
} CTAMD_API_CATCH_INT

// Number of ranked candidates for a contraction descriptor under a workspace limit (so that a
// caller can sweep CUTENSOR_PLAN_PREFERENCE_KERNEL_RANK / algo >= 0 exhaustively).
int ctamdCountCandidates(const cutensorHandle_t handle, const cutensorOperationDescriptor_t desc, uint64_t wsLimit) try {
    if (handle == nullptr || desc == nullptr || desc->kind != OpKind::Contraction) return -1;
    ContractionView v;
    if (build_contraction_view(*desc, v, nullptr) != CUTENSOR_STATUS_SUCCESS) return -1;
    if (v.dtype != HIP_R_32F || v.wide) return 0;
    return (int)rank_contraction_choices(v, wsLimit, handle->numCUs).size();
} CTAMD_API_CATCH_INT

}  // extern "C"
