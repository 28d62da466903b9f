// api.cpp — the exported cuTENSOR C ABI (include/cutensor.h) on top of the planners and the
// gfx950 kernels.  Each entry point cites the reference call site it serves.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>
#include <sstream>

#include <hip/hip_runtime.h>

#include "internal.hpp"

using namespace ctamd;

// ---- compute descriptor constants (einsum.cu:39,46,53; contraction.cu:40) ----------------------
static const cutensorComputeDescriptor kCompute[6] = {
    {0, CUTENSOR_COMPUTE_16F}, {1, CUTENSOR_COMPUTE_16BF}, {2, CUTENSOR_COMPUTE_TF32},
    {3, CUTENSOR_COMPUTE_3XTF32}, {4, CUTENSOR_COMPUTE_32F}, {5, CUTENSOR_COMPUTE_64F}};
extern "C" {
const cutensorComputeDescriptor_t CUTENSOR_COMPUTE_DESC_16F    = &kCompute[0];
const cutensorComputeDescriptor_t CUTENSOR_COMPUTE_DESC_16BF   = &kCompute[1];
const cutensorComputeDescriptor_t CUTENSOR_COMPUTE_DESC_TF32   = &kCompute[2];
const cutensorComputeDescriptor_t CUTENSOR_COMPUTE_DESC_3XTF32 = &kCompute[3];
const cutensorComputeDescriptor_t CUTENSOR_COMPUTE_DESC_32F    = &kCompute[4];
const cutensorComputeDescriptor_t CUTENSOR_COMPUTE_DESC_64F    = &kCompute[5];
}

// grid of the persistent 16-bit kernel in workgroups (0 = one per CU): CUTENSOR_AMD_H16P_GRID, a test hook — the kernel objects are
// shared by both library flavours, so the switch is read here and handed over as data (gett_h16p.hip, launch_h16w4p)
extern "C" int ctamd_h16p_grid_cap;
extern "C" int ctamd_h16p_stagger;
int ctamd_h16p_stagger = [] { const char* e = CTAMD_HOOK_ENV("CUTENSOR_AMD_H16P_STAGGER"); return e ? std::atoi(e) : -1; }();   // -1: the launcher's own step
int ctamd_h16p_grid_cap = [] { const char* e = CTAMD_HOOK_ENV("CUTENSOR_AMD_H16P_GRID"); const int v = e ? std::atoi(e) : 0; return v > 0 ? v : 0; }();

namespace {

// launches of cutensorContract by kernel kind since the library was loaded (ctamdLaunchCounts): 0 = gett_simple_kernel (scalar FMA
// fallback), 1 = gett_wide_kernel (mode table), 2 = fp32 MFMA families, 3 = aligned 16-bit MFMA family, 4 = general MFMA family
std::atomic<uint64_t> g_launchCounts[5];
std::atomic<int> g_lastH16Kernel{-1};   // table entry of the last launch of the aligned 16-bit family (ctamdLastH16Kernel: which twin ran)

bool valid_compute(cutensorComputeDescriptor_t c) { return c >= &kCompute[0] && c <= &kCompute[5]; }


bool supported_dtype(hipDataType t) {
    // complex data: contractions (general MFMA family / mode-table kernel), reductions, permutations and the binary and trinary
    // element-wise forms (ADD / MUL, operand operators IDENTITY / CONJ; the trinary form on kernels/elementwise_trinary_cplx.hip)
    return t == HIP_R_32F || t == HIP_R_64F || t == HIP_R_16F || t == HIP_R_16BF || t == HIP_C_32F || t == HIP_C_64F;
}

// scalar type of alpha/beta for a data type + compute descriptor (einsum.cu:40,47,54;
// torch/einsum.cc:39): fp64 data -> fp64 scalars, everything else -> fp32 scalars.
hipDataType scalar_type_for(hipDataType data, const cutensorComputeDescriptor* c) {
    if (data == HIP_C_32F || data == HIP_C_64F) return data;   // contraction_jit.cu:205: complex scalars for complex data
    if (data == HIP_R_64F || (c && c->id == 5)) return HIP_R_64F;
    return HIP_R_32F;
}

cutensorStatus_t fill_use(TensorUse& u, const cutensorTensorDescriptor_t d, const int32_t* modes,
                          cutensorOperator_t op) {
    if (d == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (d->numModes > 0 && modes == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    u.desc = *d;
    u.modes.assign(modes, modes + d->numModes);
    u.op = op;
    u.present = true;
    return CUTENSOR_STATUS_SUCCESS;
}

double num_elements(const cutensorTensorDescriptor& d) {
    double n = 1.0;
    for (int64_t e : d.extent) n *= (double)e;
    return n;
}

std::string problem_key(const cutensorOperationDescriptor& op) {
    std::ostringstream ss;
    ss << (int)op.kind << ':' << (int)op.A.desc.dtype << ':' << (op.compute ? op.compute->id : -1);
    // a converting element-wise problem (D's / C's type differs from A's) is another problem than the same-type one of the same shapes
    if ((op.D.present && op.D.desc.dtype != op.A.desc.dtype) || (op.C.present && op.C.desc.dtype != op.A.desc.dtype))
        ss << ":d" << (int)op.D.desc.dtype << ":c" << (op.C.present ? (int)op.C.desc.dtype : -1);
    if (op.B.present && op.B.desc.dtype != op.A.desc.dtype) ss << ":b" << (int)op.B.desc.dtype;      // a mixed fp64 x complex128 contraction
    auto put = [&](const TensorUse& u) {
        ss << '|';
        if (!u.present) return;
        for (size_t i = 0; i < u.modes.size(); ++i)
            ss << u.modes[i] << ',' << u.desc.extent[i] << ',' << u.desc.stride[i] << ';';
        ss << 'a' << u.desc.alignment;
    };
    put(op.A); put(op.B); put(op.C); put(op.D);
    return ss.str();
}

// POD memo key (internal.hpp): false when the problem is outside what the memo holds
bool build_memo_key(const cutensorOperationDescriptor& op, const cutensorPlanPreference& pr, uint64_t wsLimit, PlanMemoKey& k) {
    if (op.kind != OpKind::Contraction && op.kind != OpKind::Reduction && op.kind != OpKind::Permutation &&
        op.kind != OpKind::ElementwiseBinary) return false;
    if (!op.padLeft.empty() || !op.padRight.empty()) return false;
    const TensorUse* u[4] = {&op.A, &op.B, &op.C, &op.D};
    size_t total = 0;
    for (const TensorUse* t : u) if (t->present) total += t->modes.size();
    if (total > (size_t)PlanMemoKey::kMaxModes) return false;
    k.wsLimit = wsLimit;
    k.algo = (int32_t)pr.algo; k.kernelRank = pr.kernelRank; k.autotune = (int32_t)pr.autotune;
    k.incrementalCount = pr.autotune == CUTENSOR_AUTOTUNE_MODE_INCREMENTAL ? pr.incrementalCount : 0;
    k.operandsStreamed = (uint8_t)(pr.operandsStreamed != 0);
    k.kind = (uint8_t)op.kind; k.dtype = (uint8_t)op.A.desc.dtype; k.compute = (uint8_t)(op.compute ? op.compute->id : 255);
    k.scalarType = (uint8_t)op.scalarType;
    k.dtypeB = (op.B.present && op.B.desc.dtype != op.A.desc.dtype) ? (uint32_t)op.B.desc.dtype + 1u : 0u;
    k.dtypeD = op.D.present ? (uint8_t)op.D.desc.dtype : (uint8_t)255; k.dtypeC = op.C.present ? (uint8_t)op.C.desc.dtype : (uint8_t)255;
    k.op[0] = (uint8_t)op.A.op; k.op[1] = (uint8_t)op.B.op; k.op[2] = (uint8_t)op.C.op; k.op[3] = (uint8_t)op.opReduce;
    k.present = 0;
    uint32_t w = 0;
    for (int i = 0; i < 4; ++i) {
        const TensorUse& t = *u[i];
        k.n[i] = 0; k.alignment[i] = 0;
        if (!t.present) continue;
        k.present |= (uint8_t)(1u << i);
        const size_t n = t.modes.size();
        k.n[i] = (uint8_t)n; k.alignment[i] = t.desc.alignment;
        for (size_t j = 0; j < n; ++j) k.data[w++] = t.modes[j];
        std::memcpy(&k.data[w], t.desc.extent.data(), n * sizeof(int64_t)); w += (uint32_t)n;
        std::memcpy(&k.data[w], t.desc.stride.data(), n * sizeof(int64_t)); w += (uint32_t)n;
    }
    k.used = w;
    return true;
}

}  // namespace

uint64_t PlanMemoKey::hash() const {
    // the fixed head (everything before data[]) and the used words, 8 bytes at a time through a multiply-xorshift mix
    auto mix = [](uint64_t h, uint64_t v) { h ^= v; h *= 0x9E3779B97F4A7C15ull; return h ^ (h >> 29); };
    uint64_t h = 0xCBF29CE484222325ull;
    const size_t headWords = offsetof(PlanMemoKey, data) / 8;
    const uint64_t* p = reinterpret_cast<const uint64_t*>(this);
    for (size_t i = 0; i < headWords; ++i) h = mix(h, p[i]);
    for (uint32_t i = 0; i < used; ++i) h = mix(h, (uint64_t)data[i]);
    return h;
}
bool PlanMemoKey::operator==(const PlanMemoKey& o) const {
    return used == o.used && std::memcmp(this, &o, offsetof(PlanMemoKey, data)) == 0 &&
           std::memcmp(data, o.data, (size_t)used * sizeof(int64_t)) == 0;
}

// Incremental autotuning (contraction_plan_cache.cu:215-237): cutensorContract on a trial plan brackets its launches with
// an event pair; the pairs are read here — at the next plan creation, before the cache is written, at handle destruction —
// never inside cutensorContract, which stays asynchronous.  The fastest candidate seen so far is what the cache holds.
static void resolve_pending_measurements(cutensorHandle* handle) {
    std::vector<cutensorHandle::PendingMeasurement> todo;
    {
        std::lock_guard<std::mutex> g(handle->mtx);
        todo.swap(handle->pending);
        handle->pendingCount.store(0, std::memory_order_relaxed);
    }
    for (auto& m : todo) {
        float ms = 0.f;
        const bool ok = hipEventSynchronize(m.e1) == hipSuccess && hipEventElapsedTime(&ms, m.e0, m.e1) == hipSuccess;
        (void)hipEventDestroy(m.e0);
        (void)hipEventDestroy(m.e1);
        if (!ok) { (void)hipGetLastError(); continue; }
        std::lock_guard<std::mutex> g(handle->mtx);
        cutensorHandle::TuneState& t = handle->tuning[m.key];
        CT_LOG("incremental autotune: kernel %d splitK %u -> %.3f us (best so far %.3f us)", m.kernel, m.splitK, ms * 1e3, t.bestMs * 1e3);
        if (ms < t.bestMs) {
            t.bestMs = ms; t.bestKernel = m.kernel; t.bestSplitK = m.splitK;
            if (handle->planCache.count(m.key) || handle->planCache.size() < handle->planCacheCapacity) {
                handle->planCache[m.key] = PlanCacheEntry{m.key, m.kernel, m.splitK};
                handle->planMemo.clear();   // prototypes built from the previous best are stale
            }
        }
    }
}

// A finished plan of the kinds plan_is_prototype lists becomes the prototype later plans of the same problem are cloned from; the least
// recently used prototype makes room when the cache is full (capacity = cutensorHandleResizePlanCache's numEntries).
// A mode table, a trial's timing state or a block-sparse task list: such plans are planned every time
static bool plan_is_plain(const cutensorPlan& pl) { return pl.tuneKey.empty() && pl.wideTab.empty() && !pl.bsp; }
static bool plan_has_sub_plans(const cutensorPlan& pl) { return pl.sub1 || pl.sub2 || pl.loneA || pl.loneB; }
// Copy of a plan (it shares the source's sub-plans: SubPlan, internal.hpp)
static cutensorPlan* clone_plan(const cutensorPlan& src) { return new (std::nothrow) cutensorPlan(src); }
// What the memo holds: plain plans without sub-plans, and two-step contractions (an operand reduced over its lone modes or copied into a
// packed temporary first, then the inner contraction) whose plans are all of that kind (round 6: the planner prices up to eight copy
// combinations for them, 100-240 us per cutensorCreatePlan, and einsum.cu plans inside every call).  Peeled / trinary plans: not memoised
static bool plan_is_prototype(const cutensorPlan& pl) {
    if (!plan_is_plain(pl)) return false;
    if (!plan_has_sub_plans(pl)) return true;
    if (pl.kind != OpKind::Contraction || (pl.planKind != PlanKind::LoneReduce && pl.planKind != PlanKind::Repack) || pl.sub2 || !pl.sub1) return false;
    for (const SubPlan* q : {&pl.sub1, &pl.loneA, &pl.loneB})
        if (*q && (!plan_is_plain(**q) || plan_has_sub_plans(**q))) return false;
    return true;
}
static void memo_insert(cutensorHandle* h, const PlanMemoKey& key, uint64_t hash, const cutensorPlan& pl) {
    if (!plan_is_prototype(pl)) return;
    std::shared_ptr<const cutensorPlan> proto(clone_plan(pl));
    if (!proto) return;
    std::lock_guard<std::mutex> g(h->mtx);
    if (h->planCacheCapacity == 0) return;
    if (h->planMemo.size() >= h->planCacheCapacity && h->planMemo.find(hash) == h->planMemo.end()) {
        auto victim = h->planMemo.begin();
        for (auto it = h->planMemo.begin(); it != h->planMemo.end(); ++it)
            if (it->second.stamp < victim->second.stamp) victim = it;
        h->planMemo.erase(victim);
    }
    PlanMemoEntry& e = h->planMemo[hash];
    e.key = key; e.proto = std::move(proto); e.stamp = ++h->memoClock;
}

extern "C" {

// ---- handle (contraction.cu:123-124) -----------------------------------------------------------
cutensorStatus_t cutensorCreate(cutensorHandle_t* handle) try {
    if (handle == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorHandle* h = new (std::nothrow) cutensorHandle();
    if (h == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) {
        h->device = dev;
        h->haveDevice = true;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            h->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
            h->clockKHz = prop.clockRate > 0 ? prop.clockRate : 2400000;
            if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
                CT_LOG("warning: device is %s, kernels are built for gfx950", prop.gcnArchName);
        }
    } else {
        (void)hipGetLastError();   // no device: descriptor / planning calls still work
    }
    *handle = h;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorDestroy(cutensorHandle_t handle) try {
    if (handle != nullptr) {
        for (auto& m : handle->pending) { (void)hipEventDestroy(m.e0); (void)hipEventDestroy(m.e1); }
        for (auto& ev : handle->prof.events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    }
    if (handle != nullptr && handle->syncPool != nullptr) (void)hipFree(handle->syncPool);
    delete handle;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// einsum.cu:445
cutensorStatus_t cutensorHandleResizePlanCache(cutensorHandle_t handle, const uint32_t numEntries) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    std::lock_guard<std::mutex> g(handle->mtx);
    handle->planCacheCapacity = numEntries;
    while (handle->planCache.size() > numEntries) handle->planCache.erase(handle->planCache.begin());
    if (handle->planMemo.size() > numEntries) handle->planMemo.clear();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_plan_cache.cu:324-337 — one line per cached problem: key \t kernel \t splitK
cutensorStatus_t cutensorHandleWritePlanCacheToFile(const cutensorHandle_t handle, const char filename[]) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (filename == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    resolve_pending_measurements(handle);
    std::lock_guard<std::mutex> g(handle->mtx);
    FILE* f = std::fopen(filename, "w");
    if (f == nullptr) return CUTENSOR_STATUS_IO_ERROR;
    std::fprintf(f, "cutensor-amd-plancache 1\n");
    for (const auto& kv : handle->planCache) {   // key, kernel, splitK, candidates tried by incremental autotuning, best time [us]
        auto t = handle->tuning.find(kv.first);
        const int tried = t != handle->tuning.end() ? t->second.next : 0;
        const double us = (t != handle->tuning.end() && t->second.bestMs < 1e29f) ? t->second.bestMs * 1e3 : 0.0;
        std::fprintf(f, "%s\t%d\t%u\t%d\t%.3f\n", kv.second.key.c_str(), kv.second.kernel, kv.second.splitK, tried, us);
    }
    std::fclose(f);
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_plan_cache.cu:132-148
cutensorStatus_t cutensorHandleReadPlanCacheFromFile(cutensorHandle_t handle, const char filename[],
                                                     uint32_t* numCachelinesRead) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (filename == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (numCachelinesRead) *numCachelinesRead = 0;
    FILE* f = std::fopen(filename, "r");
    if (f == nullptr) return CUTENSOR_STATUS_IO_ERROR;
    char header[64];
    int version = 0;
    if (std::fscanf(f, "%63s %d\n", header, &version) != 2 || std::strcmp(header, "cutensor-amd-plancache") != 0) {
        std::fclose(f);
        return CUTENSOR_STATUS_IO_ERROR;
    }
    std::lock_guard<std::mutex> g(handle->mtx);
    handle->planMemo.clear();   // the file may bring a different tuned choice for a memoised problem
    std::vector<char> line(1 << 16);
    uint32_t n = 0;
    while (std::fgets(line.data(), (int)line.size(), f)) {
        char* t1 = std::strchr(line.data(), '\t');
        if (!t1) continue;
        *t1 = 0;
        PlanCacheEntry e;
        e.key = line.data();
        unsigned sk = 1;
        int tried = 0;
        double us = 0.0;
        if (std::sscanf(t1 + 1, "%d\t%u\t%d\t%lf", &e.kernel, &sk, &tried, &us) < 2) continue;
        e.splitK = sk;
        if (handle->planCache.size() >= handle->planCacheCapacity && !handle->planCache.count(e.key)) {
            std::fclose(f);
            if (numCachelinesRead) *numCachelinesRead = n;
            return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;   // cache too small for the file
        }
        handle->planCache[e.key] = e;
        if (tried > 0) {   // resume incremental autotuning where the writing process stopped
            cutensorHandle::TuneState& t = handle->tuning[e.key];
            t.next = tried; t.bestKernel = e.kernel; t.bestSplitK = e.splitK; t.bestMs = us > 0.0 ? (float)(us * 1e-3) : 1e30f;
        }
        ++n;
    }
    std::fclose(f);
    if (numCachelinesRead) *numCachelinesRead = n;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// ---- tensor descriptor (contraction.cu:131-137) ------------------------------------------------
cutensorStatus_t cutensorCreateTensorDescriptor(const cutensorHandle_t handle, cutensorTensorDescriptor_t* desc,
                                                const uint32_t numModes, const int64_t extent[],
                                                const int64_t stride[], cutensorDataType_t dataType,
                                                uint32_t alignmentRequirement) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || (numModes > 0 && extent == nullptr)) return CUTENSOR_STATUS_INVALID_VALUE;
    if (numModes > 64) return CUTENSOR_STATUS_NOT_SUPPORTED;
    if (!supported_dtype(dataType)) return CUTENSOR_STATUS_NOT_SUPPORTED;
    const size_t es = dtype_size(dataType);
    if (alignmentRequirement == 0 || alignmentRequirement % es != 0) return CUTENSOR_STATUS_INVALID_VALUE;
    std::unique_ptr<cutensorTensorDescriptor> d(new (std::nothrow) cutensorTensorDescriptor());   // owned here until it is filled
    if (d == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    d->numModes = numModes;
    d->dtype = dataType;
    d->alignment = alignmentRequirement;
    d->extent.assign(extent, extent + numModes);
    d->stride.resize(numModes);
    int64_t run = 1;
    for (uint32_t i = 0; i < numModes; ++i) {
        if (extent[i] <= 0) return CUTENSOR_STATUS_INVALID_VALUE;
        if (stride != nullptr) {
            if (stride[i] <= 0) return CUTENSOR_STATUS_INVALID_VALUE;
            d->stride[i] = stride[i];
        } else {
            d->stride[i] = run;   // packed generalized column-major (blocksparse.cu:80-81)
            run *= extent[i];
        }
    }
    *desc = d.release();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorDestroyTensorDescriptor(cutensorTensorDescriptor_t desc) try {
    delete desc;   // NULL tolerated (python/einsum.h:302,396)
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// ---- operation descriptors ----------------------------------------------------------------------
static cutensorStatus_t new_op(cutensorOperationDescriptor_t* out, cutensorOperationDescriptor& tmp) {
    cutensorOperationDescriptor* o = new (std::nothrow) cutensorOperationDescriptor(tmp);
    if (o == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    *out = o;
    return CUTENSOR_STATUS_SUCCESS;
}

// contraction.cu:162-168
cutensorStatus_t cutensorCreateContraction(const cutensorHandle_t handle, cutensorOperationDescriptor_t* desc,
                                           const cutensorTensorDescriptor_t descA, const int32_t modeA[], cutensorOperator_t opA,
                                           const cutensorTensorDescriptor_t descB, const int32_t modeB[], cutensorOperator_t opB,
                                           const cutensorTensorDescriptor_t descC, const int32_t modeC[], cutensorOperator_t opC,
                                           const cutensorTensorDescriptor_t descD, const int32_t modeD[],
                                           const cutensorComputeDescriptor_t descCompute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || !valid_compute(descCompute)) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorOperationDescriptor op{};
    op.kind = OpKind::Contraction;
    cutensorStatus_t st;
    if ((st = fill_use(op.A, descA, modeA, opA)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.B, descB, modeB, opB)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.C, descC, modeC, opC)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.D, descD, modeD, CUTENSOR_OP_IDENTITY)) != CUTENSOR_STATUS_SUCCESS) return st;
    op.compute = descCompute;
    // (a mixed contraction — one input R_64F, the other one, C and D C_64F — takes the scalars of its output: complex double)
    op.scalarType = scalar_type_for(op.A.desc.dtype != op.B.desc.dtype ? op.D.desc.dtype : op.A.desc.dtype, descCompute);
    // bytes the operation moves: every tensor at its own element size (contraction.cu:274-276)
    auto moved_bytes = [&] {
        return (double)dtype_size(op.A.desc.dtype) * num_elements(op.A.desc) + (double)dtype_size(op.B.desc.dtype) * num_elements(op.B.desc) +
               (double)dtype_size(op.D.desc.dtype) * num_elements(op.D.desc);
    };
    ContractionView v;
    std::string why;
    {
        TwoStepSplit ls;     // a mode only one input carries: validated as the reduction(s) + the contraction on the temporaries (split_lone_modes)
        if (split_lone_modes(op, ls)) {
            ReducePlan rp;
            if (ls.hasA && (st = plan_reduction(ls.stepA, 0, handle->numCUs, rp, &why)) != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreateContraction: %s", why.c_str()); return st; }
            if (ls.hasB && (st = plan_reduction(ls.stepB, 0, handle->numCUs, rp, &why)) != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreateContraction: %s", why.c_str()); return st; }
            st = build_contraction_view(ls.inner, v, &why);
            if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreateContraction: %s", why.c_str()); return st; }
            op.flops = 2.0 * (double)v.totL * (double)v.totM * (double)v.totN * (double)v.totK + (ls.hasA ? num_elements(op.A.desc) : 0.0) +
                       (ls.hasB ? num_elements(op.B.desc) : 0.0);
            op.movedBytes = moved_bytes();
            return new_op(desc, op);
        }
    }
    st = build_contraction_view(op, v, &why);
    if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreateContraction: %s", why.c_str()); return st; }
    // contraction.cu:61 / :274-276
    op.flops = 2.0 * (double)v.totL * (double)v.totM * (double)v.totN * (double)v.totK;
    op.movedBytes = moved_bytes();
    return new_op(desc, op);
} CTAMD_API_CATCH

// contraction_trinary.cu:191-198: E = alpha * A * B * C + beta * D, executed as two pairwise contractions through a
// packed intermediate T.  The pair contracted first is the one that minimises flops(first) + flops(second)
// (the sample itself states its flop count as that sum, :65-67); T keeps every mode of the pair that the third
// operand or the output still needs, in the order they appear in X then Y.
cutensorStatus_t cutensorCreateContractionTrinary(const cutensorHandle_t handle, cutensorOperationDescriptor_t* desc,
                                                  const cutensorTensorDescriptor_t descA, const int32_t modeA[], cutensorOperator_t opA,
                                                  const cutensorTensorDescriptor_t descB, const int32_t modeB[], cutensorOperator_t opB,
                                                  const cutensorTensorDescriptor_t descC, const int32_t modeC[], cutensorOperator_t opC,
                                                  const cutensorTensorDescriptor_t descD, const int32_t modeD[], cutensorOperator_t opD,
                                                  const cutensorTensorDescriptor_t descE, const int32_t modeE[],
                                                  const cutensorComputeDescriptor_t descCompute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || !valid_compute(descCompute)) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorOperationDescriptor op{};
    op.kind = OpKind::ContractionTrinary;
    cutensorStatus_t st;
    if ((st = fill_use(op.A, descA, modeA, opA)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.B, descB, modeB, opB)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.C, descC, modeC, opC)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.D, descD, modeD, opD)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.E, descE, modeE, CUTENSOR_OP_IDENTITY)) != CUTENSOR_STATUS_SUCCESS) return st;
    op.compute = descCompute;
    op.scalarType = scalar_type_for(op.A.desc.dtype, descCompute);
    for (const TensorUse* u : {&op.B, &op.C, &op.D, &op.E})      // (the mixed fp64 x complex128 rows belong to the pairwise contraction alone)
        if (u->desc.dtype != op.A.desc.dtype) { CT_LOG("cutensorCreateContractionTrinary: mixed data types"); return CUTENSOR_STATUS_NOT_SUPPORTED; }
    const TensorUse* in[3] = {&op.A, &op.B, &op.C};
    auto has = [](const std::vector<int32_t>& v, int32_t l) { return std::find(v.begin(), v.end(), l) != v.end(); };
    double bestCost = 0.0;
    bool found = false;
    static const int pairs[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};
    for (const auto& pr : pairs) {
        const TensorUse &X = *in[pr[0]], &Y = *in[pr[1]], &Z = *in[pr[2]];
        // T: modes of X and Y still needed by Z or E
        TensorUse T;
        T.present = true;
        T.desc.dtype = X.desc.dtype;
        T.desc.alignment = 128;
        double flops1 = 2.0, tElems = 1.0;
        std::vector<int32_t> seen;
        auto visit = [&](const TensorUse& U) {
            for (size_t i = 0; i < U.modes.size(); ++i) {
                const int32_t l = U.modes[i];
                if (has(seen, l)) continue;
                seen.push_back(l);
                flops1 *= (double)U.desc.extent[i];
                if (has(Z.modes, l) || has(op.E.modes, l)) {
                    T.modes.push_back(l);
                    T.desc.extent.push_back(U.desc.extent[i]);
                    tElems *= (double)U.desc.extent[i];
                }
            }
        };
        visit(X); visit(Y);
        T.desc.numModes = (uint32_t)T.modes.size();
        T.desc.stride.resize(T.modes.size());
        int64_t run = 1;
        for (size_t i = 0; i < T.modes.size(); ++i) { T.desc.stride[i] = run; run *= T.desc.extent[i]; }
        double flops2 = 2.0;
        std::vector<int32_t> seen2;
        for (const TensorUse* U : {const_cast<const TensorUse*>(&T), &Z})
            for (size_t i = 0; i < U->modes.size(); ++i)
                if (!has(seen2, U->modes[i])) { seen2.push_back(U->modes[i]); flops2 *= (double)U->desc.extent[i]; }
        cutensorOperationDescriptor s1{}, s2{};
        s1.kind = s2.kind = OpKind::Contraction;
        s1.compute = s2.compute = descCompute;
        s1.scalarType = s2.scalarType = op.scalarType;
        s1.A = X; s1.B = Y; s1.C = T; s1.D = T;
        s2.A = T; s2.B = Z; s2.C = op.D; s2.D = op.E;
        // a step is validated the way cutensorCreateContraction validates it: a mode that one of its inputs alone carries (a mode of A, B
        // or C that E lacks) makes it the reduction(s) + the contraction on the temporaries (split_lone_modes), as its plan will be
        auto step_ok = [&](const cutensorOperationDescriptor& s) {
            ContractionView v;
            std::string why;
            TwoStepSplit ls;
            if (!split_lone_modes(s, ls)) return build_contraction_view(s, v, &why) == CUTENSOR_STATUS_SUCCESS;
            ReducePlan rp;
            if (ls.hasA && plan_reduction(ls.stepA, 0, handle->numCUs, rp, &why) != CUTENSOR_STATUS_SUCCESS) return false;
            if (ls.hasB && plan_reduction(ls.stepB, 0, handle->numCUs, rp, &why) != CUTENSOR_STATUS_SUCCESS) return false;
            return build_contraction_view(ls.inner, v, &why) == CUTENSOR_STATUS_SUCCESS;
        };
        if (!step_ok(s1) || !step_ok(s2)) continue;
        s1.flops = flops1; s2.flops = flops2;
        const double cost = flops1 + flops2 + 8.0 * tElems;   // the intermediate is written and read once
        if (!found || cost < bestCost) {
            found = true;
            bestCost = cost;
            op.sub.clear();
            op.sub.push_back(s1);
            op.sub.push_back(s2);
            op.triOrder[0] = pr[0]; op.triOrder[1] = pr[1]; op.triOrder[2] = pr[2];
            op.tBytes = (uint64_t)tElems * dtype_size(T.desc.dtype);
            op.flops = flops1 + flops2;
        }
    }
    if (!found) { CT_LOG("cutensorCreateContractionTrinary: no pairwise order is supported"); return CUTENSOR_STATUS_NOT_SUPPORTED; }
    const double es = (double)dtype_size(op.A.desc.dtype);
    op.movedBytes = es * (num_elements(op.A.desc) + num_elements(op.B.desc) + num_elements(op.C.desc) + num_elements(op.E.desc));
    return new_op(desc, op);
} CTAMD_API_CATCH

// reduction.cu:141-146
cutensorStatus_t cutensorCreateReduction(const cutensorHandle_t handle, cutensorOperationDescriptor_t* desc,
                                         const cutensorTensorDescriptor_t descA, const int32_t modeA[], cutensorOperator_t opA,
                                         const cutensorTensorDescriptor_t descC, const int32_t modeC[], cutensorOperator_t opC,
                                         const cutensorTensorDescriptor_t descD, const int32_t modeD[],
                                         cutensorOperator_t opReduce, const cutensorComputeDescriptor_t descCompute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || !valid_compute(descCompute)) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorOperationDescriptor op{};
    op.kind = OpKind::Reduction;
    cutensorStatus_t st;
    if ((st = fill_use(op.A, descA, modeA, opA)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.C, descC, modeC, opC)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.D, descD, modeD, CUTENSOR_OP_IDENTITY)) != CUTENSOR_STATUS_SUCCESS) return st;
    op.opReduce = opReduce;
    op.compute = descCompute;
    op.scalarType = scalar_type_for(op.A.desc.dtype, descCompute);
    ReducePlan rp;
    std::string why;
    st = plan_reduction(op, 0, handle->numCUs, rp, &why);   // validates the problem
    if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreateReduction: %s", why.c_str()); return st; }
    const double es = (double)dtype_size(op.A.desc.dtype);
    op.flops = num_elements(op.A.desc);
    op.movedBytes = es * (num_elements(op.A.desc) + num_elements(op.D.desc));   // reduction.cu:229-231
    return new_op(desc, op);
} CTAMD_API_CATCH

// elementwise_permute.cu:142-149
cutensorStatus_t cutensorCreatePermutation(const cutensorHandle_t handle, cutensorOperationDescriptor_t* desc,
                                           const cutensorTensorDescriptor_t descA, const int32_t modeA[], cutensorOperator_t opA,
                                           const cutensorTensorDescriptor_t descB, const int32_t modeB[],
                                           const cutensorComputeDescriptor_t descCompute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || !valid_compute(descCompute)) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorOperationDescriptor op{};
    op.kind = OpKind::Permutation;
    cutensorStatus_t st;
    if ((st = fill_use(op.A, descA, modeA, opA)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.D, descB, modeB, CUTENSOR_OP_IDENTITY)) != CUTENSOR_STATUS_SUCCESS) return st;
    op.compute = descCompute;
    op.scalarType = scalar_type_for(op.A.desc.dtype, descCompute);
    EwPlan ep;
    std::string why;
    st = plan_elementwise(op, ep, &why);
    if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreatePermutation: %s", why.c_str()); return st; }
    op.movedBytes = (double)(dtype_size(op.A.desc.dtype) + dtype_size(op.D.desc.dtype)) * num_elements(op.D.desc);   // elementwise_permute.cu:208
    return new_op(desc, op);
} CTAMD_API_CATCH

// elementwise_binary.cu:149-153 — only opAC = ADD is implemented
cutensorStatus_t cutensorCreateElementwiseBinary(const cutensorHandle_t handle, cutensorOperationDescriptor_t* desc,
                                                 const cutensorTensorDescriptor_t descA, const int32_t modeA[], cutensorOperator_t opA,
                                                 const cutensorTensorDescriptor_t descC, const int32_t modeC[], cutensorOperator_t opC,
                                                 const cutensorTensorDescriptor_t descD, const int32_t modeD[],
                                                 cutensorOperator_t opAC, const cutensorComputeDescriptor_t descCompute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || !valid_compute(descCompute)) return CUTENSOR_STATUS_INVALID_VALUE;
    if (opAC != CUTENSOR_OP_ADD && opAC != CUTENSOR_OP_MUL && opAC != CUTENSOR_OP_MAX && opAC != CUTENSOR_OP_MIN) return CUTENSOR_STATUS_NOT_SUPPORTED;
    cutensorOperationDescriptor op{};
    op.kind = OpKind::ElementwiseBinary;
    cutensorStatus_t st;
    if ((st = fill_use(op.A, descA, modeA, opA)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.C, descC, modeC, opC)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.D, descD, modeD, CUTENSOR_OP_IDENTITY)) != CUTENSOR_STATUS_SUCCESS) return st;
    op.opReduce = opAC;
    op.compute = descCompute;
    op.scalarType = scalar_type_for(op.A.desc.dtype, descCompute);
    EwPlan ep;
    std::string why;
    st = plan_elementwise(op, ep, &why);
    if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreateElementwiseBinary: %s", why.c_str()); return st; }
    op.movedBytes = (double)(dtype_size(op.A.desc.dtype) + 2 * dtype_size(op.D.desc.dtype)) * num_elements(op.D.desc);
    return new_op(desc, op);
} CTAMD_API_CATCH

// elementwise_trinary.cu:174-182
cutensorStatus_t cutensorCreateElementwiseTrinary(const cutensorHandle_t handle, cutensorOperationDescriptor_t* desc,
                                                  const cutensorTensorDescriptor_t descA, const int32_t modeA[], cutensorOperator_t opA,
                                                  const cutensorTensorDescriptor_t descB, const int32_t modeB[], cutensorOperator_t opB,
                                                  const cutensorTensorDescriptor_t descC, const int32_t modeC[], cutensorOperator_t opC,
                                                  const cutensorTensorDescriptor_t descD, const int32_t modeD[],
                                                  cutensorOperator_t opAB, cutensorOperator_t opABC,
                                                  const cutensorComputeDescriptor_t descCompute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || !valid_compute(descCompute)) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorOperationDescriptor op{};
    op.kind = OpKind::ElementwiseTrinary;
    cutensorStatus_t st;
    if ((st = fill_use(op.A, descA, modeA, opA)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.B, descB, modeB, opB)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.C, descC, modeC, opC)) != CUTENSOR_STATUS_SUCCESS) return st;
    if ((st = fill_use(op.D, descD, modeD, CUTENSOR_OP_IDENTITY)) != CUTENSOR_STATUS_SUCCESS) return st;
    op.opAB = opAB;
    op.opReduce = opABC;
    op.compute = descCompute;
    op.scalarType = scalar_type_for(op.A.desc.dtype, descCompute);
    EwTrinaryPlan tp;
    std::string why;
    st = plan_elementwise_trinary(op, tp, &why);
    if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreateElementwiseTrinary: %s", why.c_str()); return st; }
    op.movedBytes = 4.0 * (double)dtype_size(op.D.desc.dtype) * num_elements(op.D.desc);   // elementwise_trinary.cu:234-238
    return new_op(desc, op);
} CTAMD_API_CATCH

cutensorStatus_t cutensorDestroyOperationDescriptor(cutensorOperationDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction.cu:176-180, contraction_jit.cu:379-383
cutensorStatus_t cutensorOperationDescriptorGetAttribute(const cutensorHandle_t handle, cutensorOperationDescriptor_t desc,
                                                         cutensorOperationDescriptorAttribute_t attr, void* buf,
                                                         size_t sizeInBytes) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || buf == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    switch (attr) {
        case CUTENSOR_OPERATION_DESCRIPTOR_TAG:
            if (sizeInBytes != sizeof(int32_t)) return CUTENSOR_STATUS_INVALID_VALUE;
            *static_cast<int32_t*>(buf) = desc->tag;
            return CUTENSOR_STATUS_SUCCESS;
        case CUTENSOR_OPERATION_DESCRIPTOR_SCALAR_TYPE:
            if (sizeInBytes != sizeof(cutensorDataType_t)) return CUTENSOR_STATUS_INVALID_VALUE;
            *static_cast<cutensorDataType_t*>(buf) = desc->scalarType;
            return CUTENSOR_STATUS_SUCCESS;
        case CUTENSOR_OPERATION_DESCRIPTOR_FLOPS:
            if (sizeInBytes != sizeof(float)) return CUTENSOR_STATUS_INVALID_VALUE;
            *static_cast<float*>(buf) = (float)desc->flops;
            return CUTENSOR_STATUS_SUCCESS;
        case CUTENSOR_OPERATION_DESCRIPTOR_MOVED_BYTES:
            if (sizeInBytes != sizeof(float)) return CUTENSOR_STATUS_INVALID_VALUE;
            *static_cast<float*>(buf) = (float)desc->movedBytes;
            return CUTENSOR_STATUS_SUCCESS;
        default:
            return CUTENSOR_STATUS_NOT_SUPPORTED;
    }
} CTAMD_API_CATCH

cutensorStatus_t cutensorOperationDescriptorSetAttribute(const cutensorHandle_t handle, cutensorOperationDescriptor_t desc,
                                                         cutensorOperationDescriptorAttribute_t attr, const void* buf,
                                                         size_t sizeInBytes) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || buf == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (attr == CUTENSOR_OPERATION_DESCRIPTOR_TAG && sizeInBytes == sizeof(int32_t)) {
        desc->tag = *static_cast<const int32_t*>(buf);
        return CUTENSOR_STATUS_SUCCESS;
    }
    // elementwise_permute_padding.cu:178-195: one int per output mode / one output-typed value
    if (attr == CUTENSOR_OPERATION_DESCRIPTOR_PADDING_LEFT || attr == CUTENSOR_OPERATION_DESCRIPTOR_PADDING_RIGHT) {
        if (desc->kind != OpKind::Permutation) return CUTENSOR_STATUS_NOT_SUPPORTED;
        if (sizeInBytes != sizeof(int32_t) * desc->D.modes.size()) return CUTENSOR_STATUS_INVALID_VALUE;
        const int32_t* v = static_cast<const int32_t*>(buf);
        std::vector<int32_t>& dst = (attr == CUTENSOR_OPERATION_DESCRIPTOR_PADDING_LEFT) ? desc->padLeft : desc->padRight;
        dst.assign(v, v + desc->D.modes.size());
        for (int32_t x : dst) if (x < 0) { dst.clear(); return CUTENSOR_STATUS_INVALID_VALUE; }
        return CUTENSOR_STATUS_SUCCESS;
    }
    if (attr == CUTENSOR_OPERATION_DESCRIPTOR_PADDING_VALUE) {
        if (desc->kind != OpKind::Permutation) return CUTENSOR_STATUS_NOT_SUPPORTED;
        if (sizeInBytes != dtype_size(desc->D.desc.dtype)) return CUTENSOR_STATUS_INVALID_VALUE;
        switch (desc->D.desc.dtype) {
            case HIP_R_32F: desc->padValue = *static_cast<const float*>(buf); break;
            case HIP_R_64F: desc->padValue = *static_cast<const double*>(buf); break;
            case HIP_R_16F: { uint16_t u; std::memcpy(&u, buf, 2); const uint32_t s = (u >> 15) & 1u, e = (u >> 10) & 31u, m = u & 1023u;
                              double x = (e == 0) ? std::ldexp((double)m, -24) : (e == 31 ? (m ? NAN : INFINITY) : std::ldexp((double)(m | 1024u), (int)e - 25));
                              desc->padValue = s ? -x : x; break; }
            case HIP_R_16BF: { uint16_t u; std::memcpy(&u, buf, 2); const uint32_t w = (uint32_t)u << 16; float f; std::memcpy(&f, &w, 4); desc->padValue = f; break; }
            default: return CUTENSOR_STATUS_NOT_SUPPORTED;
        }
        return CUTENSOR_STATUS_SUCCESS;
    }
    return CUTENSOR_STATUS_NOT_SUPPORTED;
} CTAMD_API_CATCH

// ---- plan preference (contraction.cu:194-198) ----------------------------------------------------
cutensorStatus_t cutensorCreatePlanPreference(const cutensorHandle_t handle, cutensorPlanPreference_t* pref,
                                              cutensorAlgo_t algo, cutensorJitMode_t jitMode) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (pref == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorPlanPreference* p = new (std::nothrow) cutensorPlanPreference();
    if (p == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    p->algo = algo;
    p->jit = jitMode;   // accepted and ignored: every kernel is ahead-of-time compiled for gfx950
    *pref = p;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorDestroyPlanPreference(cutensorPlanPreference_t pref) try {
    delete pref;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_plan_cache.cu:215-237
cutensorStatus_t cutensorPlanPreferenceSetAttribute(const cutensorHandle_t handle, cutensorPlanPreference_t pref,
                                                    cutensorPlanPreferenceAttribute_t attr, const void* buf,
                                                    size_t sizeInBytes) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (pref == nullptr || buf == nullptr || sizeInBytes != 4) return CUTENSOR_STATUS_INVALID_VALUE;
    const int32_t v = *static_cast<const int32_t*>(buf);
    switch (attr) {
        case CUTENSOR_PLAN_PREFERENCE_AUTOTUNE_MODE: pref->autotune = (cutensorAutotuneMode_t)v; break;
        case CUTENSOR_PLAN_PREFERENCE_CACHE_MODE: pref->cacheMode = (cutensorCacheMode_t)v; break;
        case CUTENSOR_PLAN_PREFERENCE_INCREMENTAL_COUNT: pref->incrementalCount = v; break;
        case CUTENSOR_PLAN_PREFERENCE_ALGO: pref->algo = (cutensorAlgo_t)v; break;
        case CUTENSOR_PLAN_PREFERENCE_KERNEL_RANK: pref->kernelRank = v; break;
        case CUTENSOR_PLAN_PREFERENCE_JIT: pref->jit = (cutensorJitMode_t)v; break;
        case CUTENSOR_AMD_PLAN_PREFERENCE_OPERANDS_STREAMED: pref->operandsStreamed = v != 0 ? 1 : 0; break;   // engine extension
        default: return CUTENSOR_STATUS_INVALID_VALUE;
    }
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction.cu:207-211
cutensorStatus_t cutensorEstimateWorkspaceSize(const cutensorHandle_t handle, const cutensorOperationDescriptor_t desc,
                                               const cutensorPlanPreference_t planPref,
                                               const cutensorWorksizePreference_t workspacePref,
                                               uint64_t* workspaceSizeEstimate) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || workspaceSizeEstimate == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    *workspaceSizeEstimate = 0;
    auto estimate = [&](cutensorOperationDescriptor& d, uint64_t& w) { return cutensorEstimateWorkspaceSize(handle, &d, planPref, workspacePref, &w); };
    if (desc->kind == OpKind::BlockSparseContraction) return blocksparse_estimate(handle, *desc, workspaceSizeEstimate);
    if (desc->kind == OpKind::ContractionTrinary) {   // intermediate + the larger of the two pairwise needs
        uint64_t w1 = 0, w2 = 0;
        cutensorOperationDescriptor s1 = desc->sub[0], s2 = desc->sub[1];
        F64xOffScope fullPrecision;
        cutensorStatus_t st = estimate(s1, w1);
        if (st == CUTENSOR_STATUS_SUCCESS) st = estimate(s2, w2);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        *workspaceSizeEstimate = align256(desc->tBytes) + std::max(w1, w2);
        return CUTENSOR_STATUS_SUCCESS;
    }
    TwoStepSplit ls;     // the temporaries + the largest need of the reductions and the inner contraction — at WORKSPACE_MIN too: the
    if (desc->kind == OpKind::Contraction && split_lone_modes(*desc, ls)) {     // temporaries are mandatory (the reference binding re-plans at MIN: einsum.cc:110)
        uint64_t wI = 0, wA = 0, wB = 0;
        cutensorStatus_t st = estimate(ls.inner, wI);
        if (st == CUTENSOR_STATUS_SUCCESS && ls.hasA) st = estimate(ls.stepA, wA);
        if (st == CUTENSOR_STATUS_SUCCESS && ls.hasB) st = estimate(ls.stepB, wB);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        *workspaceSizeEstimate = TwoStepLayout(ls.bytesA, ls.bytesB).offW + std::max(wI, std::max(wA, wB));
        return CUTENSOR_STATUS_SUCCESS;
    }
    if (workspacePref == CUTENSOR_WORKSPACE_MIN) return CUTENSOR_STATUS_SUCCESS;
    const uint64_t cap = (workspacePref == CUTENSOR_WORKSPACE_MAX) ? (4ull << 30) : (1ull << 30);
    if (desc->kind == OpKind::Contraction) {   // the route cutensorCreatePlan takes at the cap (contraction_route.cpp)
        const cutensorPlanPreference defaults;
        return estimate_contraction(PlanRequest{handle, *desc, planPref, planPref ? *planPref : defaults, cap}, workspacePref, workspaceSizeEstimate);
    }
    if (desc->kind == OpKind::Reduction) {
        ReducePlan rp;
        const cutensorStatus_t st = plan_reduction(*desc, cap, handle->numCUs, rp, nullptr);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        *workspaceSizeEstimate = rp.workspace;
    }
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// the fold that matches a kernel's split-K partials: accumulator-register order (fp32 ring kernels), row-major fp32, or — general family
// with 8- / 16-byte elements — row-major partials in the accumulator type
static hipError_t launch_splitk_fold(int family, const GettKernelInfo& k, const SplitKReduceParams& r, hipStream_t stream) {
    // (the mixed fp64 x complex128 kernels write complex128's double2 partials: complex128's fold takes them as they are)
    if (family == 2 && !gen_elem_f32_partials(k.elem)) return launch_gen_splitk_reduce(r, k.elem == GEN_RC64 ? (int)GEN_C64 : k.elem, stream);
    return k.fragPartials ? launch_splitk_reduce_frag(r, stream) : launch_splitk_reduce(r, stream);
}

// scratch tensors and an event pair of a measurement, released on every way out — an exception included (since round 5 the ABI turns
// bad_alloc into a status code: what it unwinds through must not leak device memory in a process that keeps running)
struct DeviceScratch {
    void *A = nullptr, *B = nullptr, *D = nullptr, *W = nullptr, *T = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~DeviceScratch() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        for (void* p : {A, B, D, W, T}) if (p) (void)hipFree(p);
    }
    // A, B, D of the operation's own spans and a workspace; A and B hold finite, non-trivial data: 0x3c3c3c3c = 0.0115f (0x3c3c: 0.0115 in
    // bf16, 1.06 in fp16)
    bool alloc(const cutensorOperationDescriptor& op, size_t wsBytes) {
        auto span = [&](const cutensorTensorDescriptor& d) { return (size_t)d.numElementsSpanned() * dtype_size(d.dtype); };
        if (hipMalloc(&A, span(op.A.desc)) != hipSuccess || hipMalloc(&B, span(op.B.desc)) != hipSuccess || hipMalloc(&D, span(op.D.desc)) != hipSuccess ||
            (wsBytes && hipMalloc(&W, wsBytes) != hipSuccess)) return false;
        (void)hipMemset(A, 0x3c, span(op.A.desc));
        (void)hipMemset(B, 0x3c, span(op.B.desc));
        return true;
    }
    // the arguments of a launch on them: D = A B
    void point(GettParams& gp, bool swapped) const {
        gp.A = swapped ? B : A; gp.B = swapped ? A : B;
        gp.endA += (unsigned long long)(uintptr_t)gp.A; gp.endB += (unsigned long long)(uintptr_t)gp.B;
        gp.C = D; gp.D = D; gp.alpha = 1.f; gp.beta = 0.f;
    }
};

// ---- measured selection for CUTENSOR_ALGO_DEFAULT_PATIENT -------------------------------------
// Times the best-ranked candidates on scratch tensors of the problem's own shape; plan creation is
// outside every timed region of the samples (contraction.cu:218-222 vs :253-270).
static int autotune_contraction(cutensorHandle_t handle, const cutensorOperationDescriptor& op,
                                const ContractionView& v, const std::vector<ContractionChoice>& ch) {
    if (ch.size() < 2) return 0;                 // nothing to choose between (the general MFMA family ranks ONE candidate)
    const int family = ch[0].family;             // 0 fp32 GETT, 1 aligned 16-bit (LDS-DMA), 2 general MFMA family — one table each
    for (const ContractionChoice& c : ch)
        if (c.family != family) return 0;        // mixed lists are not timed: a kernel index means nothing outside its own table
    uint64_t wsMax = 0;
    const size_t nTry = std::min<size_t>(ch.size(), 12);
    for (size_t i = 0; i < nTry; ++i) wsMax = std::max(wsMax, ch[i].workspace);
    DeviceScratch sc;
    void *&D = sc.D, *&W = sc.W;
    hipEvent_t &e0 = sc.e0, &e1 = sc.e1;
    int best = 0;
    if (!sc.alloc(op, wsMax) || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        (void)hipGetLastError();
        return best;
    }
    {
        int count = 0;
        const GettKernelInfo* tab = kernel_table(family, &count);
        float bestMs = 1e30f;
        for (size_t i = 0; i < nTry; ++i) {
            GettParams gp;
            SplitKReduceParams rp;
            fill_gett_params(v, ch[i], gp, rp);
            sc.point(gp, v.swapped);
            gp.partial = ch[i].splitK > 1 ? static_cast<float*>(W) : nullptr;
            rp.partial = static_cast<float*>(W); rp.C = D; rp.D = D; rp.alpha = 1.f; rp.beta = 0.f;
            // one launch = GETT kernel + (for split-K) the fold that matches the kernel's partial layout
            auto once = [&]() -> bool {
                if (tab[ch[i].kernel].launch(gp, nullptr) != hipSuccess) return false;
                return ch[i].splitK <= 1 || launch_splitk_fold(family, tab[ch[i].kernel], rp, nullptr) == hipSuccess;
            };
            if (ch[i].kernel < 0 || ch[i].kernel >= count) continue;
            float ms = 1e30f;
            bool ok = once() && hipDeviceSynchronize() == hipSuccess;
            if (ok && i == 0) {
                // clock ramp: a cold MI355X runs the first ~15-20 ms of a kernel stream ~10 % slower than its steady state
                // (DESIGN.md section 6); without this the first candidates would be timed against a handicap
                (void)hipEventRecord(e0, nullptr);
                float spent = 0.f;
                for (int guard = 0; ok && spent < 20.f && guard < 4000; ++guard) {
                    for (int r = 0; r < 8 && ok; ++r) ok = once();
                    (void)hipEventRecord(e1, nullptr);
                    ok = ok && hipEventSynchronize(e1) == hipSuccess;
                    (void)hipEventElapsedTime(&spent, e0, e1);
                }
            }
            for (int rep = 0; ok && rep < 3; ++rep) {        // best of three batches of launches issued back to back
                const int batch = 8;
                (void)hipEventRecord(e0, nullptr);
                for (int r = 0; r < batch && ok; ++r) ok = once();
                (void)hipEventRecord(e1, nullptr);
                if (!ok || hipEventSynchronize(e1) != hipSuccess) { ok = false; break; }
                float t = 0.f;
                (void)hipEventElapsedTime(&t, e0, e1);
                ms = std::min(ms, t / batch);
            }
            if (!ok) { (void)hipGetLastError(); ms = 1e30f; }
            CT_LOG("autotune: cand %zu kernel %d (%dx%dx%d) splitK %u -> %.3f us (model %.1f us)", i, ch[i].kernel,
                   tab[ch[i].kernel].bm, tab[ch[i].kernel].bn, tab[ch[i].kernel].bk, ch[i].splitK, ms * 1e3, ch[i].estimateUs);
            if (ms < bestMs) { bestMs = ms; best = (int)i; }
        }
    }
    (void)handle;
    return best;
}

// ---- per-XCD K split for one-tile split-K plans ---------------------------------------------------------------
// The eight XCDs of an MI355X sustain slightly different shader clocks under the fp32-MFMA streaming kernel
// (2.00-2.07 GHz on the parts measured, stable per part, `profiles/r01b_phase_timing_einsum.json`), and with an
// even K split the slower dies finish 1-1.5 us after the faster ones.  Once per handle the plan's own kernel is
// run on scratch tensors with its in-kernel timestamps on; the per-XCD clock (shader cycles / wall time) becomes
// the weight of that XCD's share of K.  Returns the packed tiles-per-slice bytes, 0 = keep the uniform split.
static unsigned long long calibrate_xcd_split(cutensorHandle_t handle, const cutensorOperationDescriptor& op, const cutensorPlan& pl) {
    const uint32_t splitK = pl.gett.splitK;
    if (pl.gett.nBlocks != splitK || splitK % 8 != 0 || splitK > (uint32_t)handle->numCUs) return 0;
    int count = 0;
    const GettKernelInfo* tab = gett_f32_kernels(&count);
    const GettKernelInfo& k = tab[pl.choice.kernel];
    const uint64_t kTiles = pl.view.totK / k.bk;
    const uint64_t perXcdSum = kTiles / (splitK / 8);            // sum over x of tiles-per-slice(x)
    if (kTiles % (splitK / 8) != 0 || perXcdSum / 8 < 8 || perXcdSum / 8 > 200) return 0;
    {
        std::lock_guard<std::mutex> g(handle->mtx);
        if (handle->xcdSpeed.empty()) {
            handle->xcdSpeed.assign(8, 1.0);
            DeviceScratch sc;
            void *&W = sc.W, *&T = sc.T;
            const size_t tBytes = (size_t)splitK * 16 * sizeof(unsigned long long);
            std::vector<unsigned long long> host((size_t)splitK * 16);
            bool ok = sc.alloc(op, pl.requiredWorkspace) && hipMalloc(&T, tBytes) == hipSuccess;
            if (ok) {
                (void)hipMemset(T, 0, tBytes);
                GettParams gp = pl.gett;
                sc.point(gp, pl.view.swapped);
                gp.partial = static_cast<float*>(W);
                gp.sync = nullptr;
                gp.xcdTiles = 0;
                for (int rep = 0; rep < 4 && ok; ++rep) {
                    gp.timing = (rep == 3) ? static_cast<unsigned long long*>(T) : nullptr;
                    ok = k.launch(gp, nullptr) == hipSuccess;
                }
                ok = ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(host.data(), T, tBytes, hipMemcpyDeviceToHost) == hipSuccess;
            }
            if (ok) {
                // workgroup b runs on XCD b % 8 (observed placement; only the weights depend on it)
                double clk[8] = {0}, n[8] = {0};
                for (uint32_t b = 0; b < splitK; ++b) {
                    const unsigned long long* t = &host[(size_t)b * 16];
                    const double cyc = (double)(t[4] - t[0]), wall = (double)(t[6] - t[5]);
                    if (t[4] > t[0] && t[6] > t[5]) { clk[b & 7] += cyc / wall; n[b & 7] += 1.0; }
                }
                double mean = 0.0;
                bool all = true;
                for (int x = 0; x < 8; ++x) { all = all && n[x] > 0; if (n[x] > 0) clk[x] /= n[x]; mean += clk[x] / 8.0; }
                if (all && mean > 0)
                    for (int x = 0; x < 8; ++x) {
                        const double w = clk[x] / mean;
                        handle->xcdSpeed[x] = (w > 0.9 && w < 1.1) ? w : 1.0;   // a die 10 % off is a measurement artefact
                    }
                CT_LOG("xcd calibration: relative clocks %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f", handle->xcdSpeed[0], handle->xcdSpeed[1],
                       handle->xcdSpeed[2], handle->xcdSpeed[3], handle->xcdSpeed[4], handle->xcdSpeed[5], handle->xcdSpeed[6], handle->xcdSpeed[7]);
            } else {
                (void)hipGetLastError();
            }
        }
    }
    // largest-remainder apportionment of perXcdSum tiles
    double sum = 0.0;
    for (double w : handle->xcdSpeed) sum += w;
    uint32_t n[8];
    double frac[8];
    uint64_t assigned = 0;
    for (int x = 0; x < 8; ++x) {
        const double ideal = (double)perXcdSum * handle->xcdSpeed[x] / sum;
        n[x] = (uint32_t)ideal;
        frac[x] = ideal - n[x];
        assigned += n[x];
    }
    while (assigned < perXcdSum) {
        int best = 0;
        for (int x = 1; x < 8; ++x) if (frac[x] > frac[best]) best = x;
        n[best] += 1; frac[best] = -1.0; assigned += 1;
    }
    unsigned long long packed = 0;
    bool uniform = true;
    for (int x = 0; x < 8; ++x) {
        if (n[x] == 0 || n[x] > 255) return 0;
        uniform = uniform && n[x] == n[0];
        packed |= (unsigned long long)n[x] << (8 * x);
    }
    return uniform ? 0 : packed;
}

// ---- plan builders ------------------------------------------------------------------------------------------------
// A builder that returns `Built` answers nothing when the problem is not of its kind (the next
// builder looks at it), else how building the plan went.  Sub-plans are created through cutensorCreatePlan itself (they go through the
// plan memo like any other plan) and are owned by `pl` or by a local from the start.
using Built = std::optional<cutensorStatus_t>;
static cutensorStatus_t create_sub_plan(const PlanRequest& rq, cutensorOperationDescriptor& d, uint64_t wsLimit, SubPlan& out) {
    cutensorPlan_t p = nullptr;
    const cutensorStatus_t st = cutensorCreatePlan(rq.handle, &p, &d, rq.pref, wsLimit);
    out.reset(p);
    return st;
}
// a plan the host loops of a peeled contraction can launch: one launch of a tiled (or the simple) kernel
static bool plan_is_one_launch(const SubPlan& p) { return p->planKind != PlanKind::ModeTable && !p->sub1; }

// E = alpha A B C + beta D: two pairwise plans and the intermediate at the head of the workspace
static cutensorStatus_t build_trinary(const PlanRequest& rq, cutensorPlan& pl) {
    const cutensorOperationDescriptor& desc = rq.desc;
    const uint64_t tOff = align256(desc.tBytes);
    if (rq.wsLimit < tOff) { CT_LOG("cutensorCreatePlan: trinary contraction needs %llu bytes for its intermediate", (unsigned long long)tOff); return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE; }
    cutensorOperationDescriptor s1 = desc.sub[0], s2 = desc.sub[1];
    F64xOffScope fullPrecision;
    cutensorStatus_t st = create_sub_plan(rq, s1, rq.wsLimit - tOff, pl.sub1);
    if (st == CUTENSOR_STATUS_SUCCESS) st = create_sub_plan(rq, s2, rq.wsLimit - tOff, pl.sub2);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    pl.tBytes = desc.tBytes;
    for (int i = 0; i < 3; ++i) pl.triOrder[i] = desc.triOrder[i];
    pl.alignB3 = desc.B.desc.alignment;            // B
    pl.alignC = desc.C.desc.alignment;             // C (third input)
    pl.alignD = desc.E.desc.alignment;             // output E (and its beta source D)
    pl.requiredWorkspace = tOff + std::max(pl.sub1->requiredWorkspace, pl.sub2->requiredWorkspace);
    return CUTENSOR_STATUS_SUCCESS;
}
// a mode that one input alone carries (split_lone_modes): reduce the operand(s) over it into packed temporaries at the head of the
// workspace, then contract
static Built build_lone_reduce(const PlanRequest& rq, cutensorPlan& pl) {
    TwoStepSplit ls;
    if (!split_lone_modes(rq.desc, ls)) return {};
    const TwoStepLayout lay(ls.bytesA, ls.bytesB);
    if (rq.wsLimit < lay.offW) {
        CT_LOG("cutensorCreatePlan: a contraction with a mode that one input alone carries needs %llu bytes for its temporaries", (unsigned long long)lay.offW);
        return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
    }
    cutensorStatus_t st = create_sub_plan(rq, ls.inner, rq.wsLimit - lay.offW, pl.sub1);
    if (st == CUTENSOR_STATUS_SUCCESS && ls.hasA) st = create_sub_plan(rq, ls.stepA, rq.wsLimit - lay.offW, pl.loneA);
    if (st == CUTENSOR_STATUS_SUCCESS && ls.hasB) st = create_sub_plan(rq, ls.stepB, rq.wsLimit - lay.offW, pl.loneB);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    pl.loneBytesA = ls.bytesA; pl.loneBytesB = ls.bytesB;
    if (rq.desc.A.desc.dtype == HIP_R_16F && rq.desc.scalarType == HIP_R_32F) {   // (loneShiftA: internal.hpp)
        auto ceil_log2 = [](int64_t n) { int s = 0; while ((int64_t{1} << s) < n) ++s; return s; };
        pl.loneShiftA = ls.hasA ? (ceil_log2(ls.summedA) + 1) / 2 : 0;
        pl.loneShiftB = ls.hasB ? (ceil_log2(ls.summedB) + 1) / 2 : 0;
    }
    pl.planKind = PlanKind::LoneReduce;
    pl.requiredWorkspace = lay.offW + std::max<uint64_t>(pl.sub1->requiredWorkspace, std::max<uint64_t>(pl.loneA ? pl.loneA->requiredWorkspace : 0, pl.loneB ? pl.loneB->requiredWorkspace : 0));
    CT_LOG("plan: contraction with modes that one input alone carries -> %s%sreduced first (%llu + %llu bytes of temporaries), then the contraction",
           pl.loneA ? "A " : "", pl.loneB ? "B " : "", (unsigned long long)ls.bytesA, (unsigned long long)ls.bytesB);
    return CUTENSOR_STATUS_SUCCESS;
}
// too many unfusable modes in a group for the tiled kernels (route_peeled): the smallest ones peeled into a host loop around the inner
// plan; else the mode-table kernel takes the problem
static Built build_peeled(const PlanRequest& rq, cutensorPlan& pl) {
    cutensorOperationDescriptor inner;
    std::vector<PeelMode> peel;
    if (!route_peeled(rq, pl.view, inner, peel)) return {};
    SubPlan ip, ip2;
    if (create_sub_plan(rq, inner, rq.wsLimit, ip) != CUTENSOR_STATUS_SUCCESS || !plan_is_one_launch(ip)) return {};
    // A peeled CONTRACTED mode accumulates into D: every launch after the first reads D as its C operand.  The inner plan carries the
    // caller's C layout (and its conjugation); when that differs from D's, the accumulate launches get a second inner plan whose C
    // descriptor is D's.
    bool contracted = false;
    int64_t launches = 1;
    for (const PeelMode& pm : peel) { contracted = contracted || pm.contracted; launches *= pm.extent; }
    if (contracted && (inner.C.desc.stride != inner.D.desc.stride || inner.C.op != CUTENSOR_OP_IDENTITY)) {
        cutensorOperationDescriptor inner2 = inner;
        inner2.C = inner.D;
        inner2.C.op = CUTENSOR_OP_IDENTITY;
        if (create_sub_plan(rq, inner2, rq.wsLimit, ip2) != CUTENSOR_STATUS_SUCCESS || !plan_is_one_launch(ip2)) return CUTENSOR_STATUS_NOT_SUPPORTED;
        ip->requiredWorkspace = std::max(ip->requiredWorkspace, ip2->requiredWorkspace);
    }
    pl.requiredWorkspace = ip->requiredWorkspace;
    pl.sub1 = std::move(ip);
    pl.sub2 = std::move(ip2);
    pl.peel = peel;
    pl.planKind = PlanKind::Peeled;
    CT_LOG("plan: contraction with an oversized mode group -> %zu mode(s) peeled, %lld launches of the tiled inner plan", peel.size(), (long long)launches);
    return CUTENSOR_STATUS_SUCCESS;
}
// conjugation flags follow the operands into their kernel roles (kernel-A is the user's B when swapped)
static void set_conjugation(const cutensorOperationDescriptor& desc, bool swapped, int32_t& conjA, int32_t& conjB, int32_t& conjC) {
    const bool cA = desc.A.op == CUTENSOR_OP_CONJ, cB = desc.B.op == CUTENSOR_OP_CONJ;
    conjA = swapped ? cB : cA;
    conjB = swapped ? cA : cB;
    conjC = desc.C.op == CUTENSOR_OP_CONJ;
}
// the mode table of a plan in device memory (null: no memory, or no device)
static std::shared_ptr<const WideMode> upload_mode_table(const std::vector<WideMode>& tab) {
    void* dev = nullptr;
    const size_t bytes = tab.size() * sizeof(WideMode);
    std::shared_ptr<const WideMode> owner;
    if (hipMalloc(&dev, bytes) == hipSuccess) owner.reset(static_cast<const WideMode*>(dev), [](const WideMode* p) { (void)hipFree(const_cast<WideMode*>(p)); });
    if (owner && hipMemcpy(dev, tab.data(), bytes, hipMemcpyHostToDevice) == hipSuccess) return owner;
    (void)hipGetLastError();
    return nullptr;
}
// mode-table kernel (route_mode_table): output modes (L, M, N), then contracted modes, in device memory owned by the plan
static Built build_mode_table(const PlanRequest& rq, cutensorPlan& pl) {
    if (!route_mode_table(rq, pl.view, pl.accumulate64)) return {};
    const ContractionView& v = pl.view;
    std::vector<WideMode>& tab = pl.wideTab;
    uint64_t outTotal = 1;
    for (const std::vector<CanonMode>* g : {&v.L, &v.M, &v.N})
        for (const CanonMode& m : *g) {
            tab.push_back(WideMode{make_fastdiv((uint32_t)m.extent), m.sA, m.sB, m.sC, m.sD});
            outTotal *= (uint64_t)m.extent;
        }
    pl.wide.nOut = (uint32_t)tab.size();
    for (const CanonMode& m : v.K) tab.push_back(WideMode{make_fastdiv((uint32_t)m.extent), m.sA, m.sB, 0, 0});
    pl.wide.nK = (uint32_t)v.K.size();
    pl.wide.outTotal = outTotal;
    pl.wide.kTotal = (uint32_t)v.totK;
    set_conjugation(rq.desc, v.swapped, pl.wide.conjA, pl.wide.conjB, pl.wide.conjC);
    pl.wide.realOperand = v.realSide + 1;      // a mixed fp64 x complex128 contraction: the kernel reads that input as doubles
    if (tab.empty()) tab.push_back(WideMode{make_fastdiv(1), 0, 0, 0, 0});
    // The table goes to device memory HERE when the handle has a device — on the handle's device, outside any stream capture, so that
    // cutensorContract neither allocates nor synchronises (it may be called while a graph is being captured).  Handles without a
    // device (plan-only, the CPU tests) keep the host copy: planning needs no GPU, and a plan that one of those hands to a process
    // with a GPU uploads at first execution (launch_mode_table).
    if (rq.handle->haveDevice) {
        int prev = -1;
        const bool switched = hipGetDevice(&prev) == hipSuccess && prev != rq.handle->device && hipSetDevice(rq.handle->device) == hipSuccess;
        pl.wideDev = upload_mode_table(tab);
        if (switched) (void)hipSetDevice(prev);
    }
    pl.planKind = PlanKind::ModeTable;
    pl.requiredWorkspace = 0;
    CT_LOG("plan: contraction with %u output + %u contracted unfusable modes -> mode-table kernel", pl.wide.nOut, pl.wide.nK);
    return CUTENSOR_STATUS_SUCCESS;
}
// operands copied into packed temporaries first (route_repack), then the contraction on the temporaries
static Built build_repack(const PlanRequest& rq, cutensorPlan& pl, const TiledRoute& r) {
    TwoStepSplit rs;
    if (!route_repack(rq, pl.view, r, rs)) return {};
    const TwoStepLayout lay(rs.bytesA, rs.bytesB);
    SubPlan pi, pa, pb;
    cutensorStatus_t st;
    {
        RepackScope scope;
        st = create_sub_plan(rq, rs.inner, rq.wsLimit - lay.offW, pi);
    }
    if (st == CUTENSOR_STATUS_SUCCESS && rs.hasA) st = create_sub_plan(rq, rs.stepA, 0, pa);
    if (st == CUTENSOR_STATUS_SUCCESS && rs.hasB) st = create_sub_plan(rq, rs.stepB, 0, pb);
    // (the copies or the inner plan refused: the general family takes the problem as it is)
    if (st != CUTENSOR_STATUS_SUCCESS || pi->choice.family != r.family() || pi->sub1) return {};
    pl.requiredWorkspace = lay.offW + pi->requiredWorkspace;
    pl.sub1 = std::move(pi); pl.loneA = std::move(pa); pl.loneB = std::move(pb);
    pl.loneBytesA = rs.bytesA; pl.loneBytesB = rs.bytesB;
    pl.planKind = PlanKind::Repack;
    CT_LOG("plan: 16-bit contraction whose operands the LDS-DMA kernels cannot stage -> %s%scopied into packed temporaries first (%llu + %llu bytes), then the contraction",
           pl.loneA ? "A " : "", pl.loneB ? "B " : "", (unsigned long long)rs.bytesA, (unsigned long long)rs.bytesB);
    return CUTENSOR_STATUS_SUCCESS;
}
// Which of the ranked candidates `ch` (not empty) the plan takes: an incremental-autotuning trial, the plan cache's entry, the
// candidate the caller names, the measured one (PATIENT) — else the first
static size_t select_candidate(const PlanRequest& rq, cutensorPlan& pl, const std::vector<ContractionChoice>& ch) {
    cutensorHandle* handle = rq.handle;
    const cutensorPlanPreference& pr = rq.pr;
    size_t idx = 0;
    // (a plan made under the "operands are streamed" preference neither reads nor feeds the per-problem cache: the cache is keyed by
    // the problem alone, and its entry belongs to the default policy)
    const bool useCache = handle->planCacheCapacity > 0 && pr.cacheMode != CUTENSOR_CACHE_MODE_NONE && pr.operandsStreamed == 0;
    const bool explicitPick = names_candidate(pr);   // the caller names a candidate: the cache has no say
    const bool incremental = useCache && !explicitPick && pr.autotune == CUTENSOR_AUTOTUNE_MODE_INCREMENTAL;
    const bool patient = pr.algo == CUTENSOR_ALGO_DEFAULT_PATIENT;
    bool needKey = incremental || (useCache && patient);
    if (useCache && !explicitPick && !needKey) {
        std::lock_guard<std::mutex> g(handle->mtx);
        needKey = !handle->planCache.empty();
    }
    const std::string key = needKey ? problem_key(rq.desc) : std::string();   // the string form is what the cache FILE holds
    // incremental autotuning (contraction_plan_cache.cu:215-237): the first INCREMENTAL_COUNT plans of a problem
    // are trials of candidates 0, 1, ... (timed by cutensorContract: the best of a trial plan's first few executions);
    // after that — and for every plan without the autotune mode — the cache answers with the fastest candidate
    // measured so far.  (The sample's loop is count + 1 rounds of which the last must hit the cache, :262.)
    if (incremental) {
        resolve_pending_measurements(handle);
        std::lock_guard<std::mutex> g(handle->mtx);
        auto tit = handle->tuning.find(key);
        if (tit == handle->tuning.end() && handle->tuning.size() < std::max<size_t>(handle->planCacheCapacity, 1))
            tit = handle->tuning.emplace(key, cutensorHandle::TuneState{}).first;   // bounded like the cache itself
        if (tit != handle->tuning.end()) {
            cutensorHandle::TuneState& t = tit->second;
            const int limit = std::min<int>(std::max<int32_t>(pr.incrementalCount, 1), (int)ch.size());
            if (t.next < limit) {
                pl.tuneKey = key;
                return (size_t)t.next++;
            }
        }
    }
    if (useCache && !explicitPick) {
        std::lock_guard<std::mutex> g(handle->mtx);
        auto it = needKey ? handle->planCache.find(key) : handle->planCache.end();
        if (it != handle->planCache.end())
            for (size_t i = 0; i < ch.size(); ++i)
                if (ch[i].kernel == it->second.kernel && ch[i].splitK == it->second.splitK) return i;
    }
    if ((int)pr.algo >= 0) idx = std::min<size_t>((size_t)pr.algo, ch.size() - 1);
    else if (pr.kernelRank > 0) idx = std::min<size_t>((size_t)pr.kernelRank, ch.size() - 1);
    else if (patient) idx = (size_t)autotune_contraction(handle, rq.desc, pl.view, ch);
    if (const char* f = CTAMD_HOOK_ENV("CUTENSOR_AMD_FORCE")) {   // "kernel:splitK" experiment knob
        int fk = -1; unsigned fs = 1;
        if (std::sscanf(f, "%d:%u", &fk, &fs) >= 1)
            for (size_t i = 0; i < ch.size(); ++i)
                if (ch[i].kernel == fk && ch[i].splitK == fs) { idx = i; break; }
    }
    if (useCache && patient) {
        std::lock_guard<std::mutex> g(handle->mtx);
        if (handle->planCache.size() < handle->planCacheCapacity) {
            handle->planCache[key] = PlanCacheEntry{key, ch[idx].kernel, ch[idx].splitK};
            handle->planMemo.clear();   // a DEFAULT prototype memoised earlier must not shadow the measured choice
        }
    }
    return idx;
}
// the two opt-in refinements of a split-K plan on the fp32 ring kernels: a per-XCD K split and the in-launch fold
static void tune_f32_splitk(const PlanRequest& rq, cutensorPlan& pl) {
    const ContractionChoice& pick = pl.choice;
    if (pl.planKind != PlanKind::Tiled || pick.family != 0 || pick.splitK <= 1) return;
    const GettKernelInfo& k = *kernel_info(0, pick.kernel);
    if (!k.fragPartials || k.ablation) return;
    // Per-XCD K split (one output tile, split-K over whole XCD rows): see calibrate_xcd_split.  Opt-in: on the parts measured the clocks
    // differ by +-1.5 %, below the 1-tile-in-32 (3 %) granularity of the headline split, so the apportionment comes out uniform
    // 
    if (pick.splitK >= 64 && pl.view.totL == 1 && pl.gett.tilesM * pl.gett.tilesN == 1) {
        const char* env = CTAMD_HOOK_ENV("CUTENSOR_AMD_XCD_BALANCE");
        if (env && env[0] == '1') pl.gett.xcdTiles = calibrate_xcd_split(rq.handle, rq.desc, pl);
    }
    // In-launch fold of the split-K partials: only when every workgroup of the launch owns a CU of its own (they wait for each other)
    // and the output is a plain matrix; otherwise the fold is a second kernel.  Opt-in: measured slower than the two-kernel fold
    if (CTAMD_HOOK_ENV_IS("CUTENSOR_AMD_FUSED_FOLD", '1') && pl.gett.nBlocks <= (uint32_t)rq.handle->numCUs && pl.view.totL == 1 &&
        pl.view.M.size() <= 1 && pl.view.N.size() <= 1) {
        std::lock_guard<std::mutex> g(rq.handle->mtx);
        if (rq.handle->syncPool == nullptr) {
            void* ptr = nullptr;
            const size_t bytes = (size_t)cutensorHandle::kSyncSlots * 64;
            if (hipMalloc(&ptr, bytes) == hipSuccess && hipMemset(ptr, 0, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess)
                rq.handle->syncPool = static_cast<uint32_t*>(ptr);
            else
                (void)hipGetLastError();
        }
        pl.fusedFold = rq.handle->syncPool != nullptr;
    }
}
static void log_tiled_plan(const cutensorPlan& pl) {
    if (log_level() <= 0) return;
    const ContractionView& v = pl.view;
    const ContractionChoice& pick = pl.choice;
    const unsigned long long L = v.totL, M = v.totM, N = v.totN, K = v.totK;
    if (pl.planKind == PlanKind::Simple) { CT_LOG("plan: contraction -> simple kernel (dtype %d)", (int)v.dtype); return; }
    const GettKernelInfo& k = *kernel_info(pick.family, pick.kernel);
    if (pick.family == 2)
        CT_LOG("plan: contraction (general MFMA family) dtype=%d L=%llu M=%llu N=%llu K=%llu swapped=%d -> gen kernel %d (%dx%dx%d orientA=%d orientB=%d V=%d) splitK=%u",
               (int)v.dtype, L, M, N, K, (int)v.swapped, pick.kernel, k.bm, k.bn, k.bk, k.layA, k.layB, k.vec, pick.splitK);
    else if (pick.family == 1)
        CT_LOG("plan: contraction (16-bit MFMA) L=%llu M=%llu N=%llu K=%llu layA=%d layB=%d swapped=%d -> h16 kernel %d", L, M, N, K, v.layA, v.layB,
               (int)v.swapped, pick.kernel);
    else
        CT_LOG("plan: contraction L=%llu M=%llu N=%llu K=%llu layA=%d layB=%d swapped=%d -> kernel %d (%dx%dx%d) splitK=%u ws=%llu est=%.1fus", L, M, N, K,
               v.layA, v.layB, (int)v.swapped, pick.kernel, k.bm, k.bn, k.bk, pick.splitK, (unsigned long long)pick.workspace, pick.estimateUs);
}
// one launch of a tiled kernel (+ the split-K fold), or of the simple kernel when no family has a candidate
static cutensorStatus_t build_tiled(const PlanRequest& rq, cutensorPlan& pl, TiledRoute& r) {
    route_tiled(rq, pl.view, r);
    if (!r.ch.empty()) pl.choice = r.ch[select_candidate(rq, pl, r.ch)];
    pl.planKind = pl.choice.kernel >= 0 ? PlanKind::Tiled : PlanKind::Simple;
    // a one-tile split-K plan of the streaming fp32 kernel: the contracted digits in the order its operand stream prefers (the choice stands)
    std::vector<CanonMode> kOrder;
    if (r.mfmaPath && pl.planKind == PlanKind::Tiled && stream_k_order(pl.view, pl.choice, kOrder)) pl.view.K = std::move(kOrder);
    fill_gett_params(pl.view, pl.choice, pl.gett, pl.skr);
    set_conjugation(rq.desc, pl.view.swapped, pl.gett.conjA, pl.gett.conjB, pl.gett.conjC);
    pl.requiredWorkspace = pl.choice.workspace;
    if (r.mfmaPath) tune_f32_splitk(rq, pl);
    log_tiled_plan(pl);
    return CUTENSOR_STATUS_SUCCESS;
}
// one builder per route, in the order of contraction_route.cpp (estimate_contraction walks the same routes without building plans)
static cutensorStatus_t build_contraction(const PlanRequest& rq, cutensorPlan& pl) {
    if (const Built b = build_lone_reduce(rq, pl)) return *b;
    const cutensorStatus_t st = build_contraction_view(rq.desc, pl.view, nullptr);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    if (const Built b = build_peeled(rq, pl)) return *b;
    if (const Built b = build_mode_table(rq, pl)) return *b;
    TiledRoute r = rank_tiled_candidates(rq, pl.view, pl.accumulate64);
    for (const std::string& line : r.notes) CT_LOG("%s", line.c_str());
    if (const Built b = build_repack(rq, pl, r)) return *b;
    return build_tiled(rq, pl, r);
}
// The output buffer of a padded permutation is the packed tensor of extents e + padLeft + padRight (the sample sizes it that way,
// elementwise_permute_padding.cu:101-103); the descriptor carries the unpadded extents.
static cutensorStatus_t build_padded_permutation(const PlanRequest& rq, cutensorPlan& pl) {
    const cutensorOperationDescriptor& desc = rq.desc;
    const size_t nm = desc.D.modes.size();
    std::vector<int64_t> padded(nm);
    int64_t accU = 1, accP = 1, offset = 0;
    bool isPacked = true;
    for (size_t i = 0; i < nm; ++i) {
        const int64_t l = desc.padLeft.empty() ? 0 : desc.padLeft[i], r = desc.padRight.empty() ? 0 : desc.padRight[i];
        padded[i] = accP;
        isPacked = isPacked && (desc.D.desc.extent[i] == 1 || desc.D.desc.stride[i] == accU);
        offset += l * accP;
        accU *= desc.D.desc.extent[i];
        accP *= desc.D.desc.extent[i] + l + r;
    }
    if (!isPacked) { CT_LOG("cutensorCreatePlan: padding needs a packed output descriptor"); return CUTENSOR_STATUS_NOT_SUPPORTED; }
    cutensorOperationDescriptor inner = desc;
    inner.D.desc.stride = padded;
    // the interior starts `offset` elements into the buffer: keep the 16-byte-lane variants only if that is lane-aligned
    // (a converting permutation: the lane of the pair, 16 bytes of the narrower type)
    const int64_t lane = 16 / (int64_t)std::min(dtype_size(desc.D.desc.dtype), dtype_size(desc.A.desc.dtype));
    if (offset % lane != 0) inner.D.desc.alignment = (uint32_t)dtype_size(desc.D.desc.dtype);
    const cutensorStatus_t st = plan_elementwise(inner, pl.ew, nullptr);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    pl.padFillElems = (uint64_t)accP;
    pl.padOffsetElems = offset;
    pl.padValue = desc.padValue;
    CT_LOG("plan: padded permutation variant=%d fill=%llu elems offset=%lld", pl.ew.variant, (unsigned long long)pl.padFillElems, (long long)offset);
    return CUTENSOR_STATUS_SUCCESS;
}
// element-wise operations and reductions: one planner call each
static cutensorStatus_t build_elementwise(const PlanRequest& rq, cutensorPlan& pl) {
    const cutensorOperationDescriptor& desc = rq.desc;
    if (desc.kind == OpKind::Reduction) {
        const cutensorStatus_t st = plan_reduction(desc, rq.wsLimit, rq.handle->numCUs, pl.red, nullptr);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        pl.requiredWorkspace = pl.red.workspace;
        CT_LOG("plan: reduction variant=%d kept=%u red=%u splitR=%u perm=%d", pl.red.variant, pl.red.p.kept.total, pl.red.p.red.total, pl.red.p.splitR,
               (int)pl.red.isPermutation);
    } else if (desc.kind == OpKind::ElementwiseTrinary) {
        const cutensorStatus_t st = plan_elementwise_trinary(desc, pl.ew3, nullptr);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        pl.alignB3 = desc.B.desc.alignment;
        CT_LOG("plan: elementwise trinary passes=%d swapAB=%d bothPermuted=%d variant(last)=%d", pl.ew3.twoPass ? 2 : 1, (int)pl.ew3.swapAB,
               (int)pl.ew3.bothPermuted, pl.ew3.last.variant);
    } else {
        const cutensorStatus_t st = plan_elementwise(desc, pl.ew, nullptr);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        CT_LOG("plan: elementwise variant=%d E0=%u E1=%u rest=%u blocks=%u", pl.ew.variant, pl.ew.p.E0, pl.ew.p.E1, pl.ew.p.rest.total, pl.ew.p.nBlocks);
    }
    return CUTENSOR_STATUS_SUCCESS;
}
static cutensorStatus_t build_plan(const PlanRequest& rq, cutensorPlan& pl) {
    switch (rq.desc.kind) {
        case OpKind::BlockSparseContraction: return blocksparse_plan(rq.handle, rq.desc, rq.wsLimit, &pl);
        case OpKind::ContractionTrinary:     return build_trinary(rq, pl);
        case OpKind::Contraction:            return build_contraction(rq, pl);
        default:   // reductions and the element-wise operations; CUTENSOR_OPERATION_DESCRIPTOR_PADDING_* is accepted on permutations only
            return (rq.desc.padLeft.empty() && rq.desc.padRight.empty()) ? build_elementwise(rq, pl) : build_padded_permutation(rq, pl);
    }
}

// contraction.cu:218-222, elementwise_permute.cu:183-187 (limit 0), einsum.cu:324-329 (limit 1 GiB)
cutensorStatus_t cutensorCreatePlan(const cutensorHandle_t handle, cutensorPlan_t* plan,
                                    const cutensorOperationDescriptor_t desc, const cutensorPlanPreference_t pref,
                                    uint64_t workspaceSizeLimit) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || desc == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorPlanPreference defaults;
    const cutensorPlanPreference& pr = pref ? *pref : defaults;
    // Plan memo first (einsum.cu:264-329 plans inside every call with the cache on, :443-445): a repeated problem is one
    // hash + one lookup + one clone; ranking candidates, string keys and tile arithmetic happen on a miss only.
    PlanMemoKey mkey;
    uint64_t mhash = 0;
    const bool memoable = handle->planCacheCapacity > 0 && pr.cacheMode != CUTENSOR_CACHE_MODE_NONE && !plan_env_override() &&
                          !(t_f64xOff > 0 && f64x_elem_of(*desc) >= 0) && build_memo_key(*desc, pr, workspaceSizeLimit, mkey);
    if (memoable) {
        mhash = mkey.hash();
        if (handle->pendingCount.load(std::memory_order_relaxed) > 0) resolve_pending_measurements(handle);
        std::shared_ptr<const cutensorPlan> proto;
        {
            std::lock_guard<std::mutex> g(handle->mtx);
            auto it = handle->planMemo.find(mhash);
            if (it != handle->planMemo.end() && it->second.key == mkey) {
                proto = it->second.proto;
                it->second.stamp = ++handle->memoClock;
            }
        }
        if (proto) {
            cutensorPlan* clone = clone_plan(*proto);
            if (clone == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
            handle->memoHits.fetch_add(1, std::memory_order_relaxed);
            *plan = clone;
            return CUTENSOR_STATUS_SUCCESS;
        }
        handle->memoMisses.fetch_add(1, std::memory_order_relaxed);
    }
    // the plan under construction is owned here until it is handed to the caller: an exception below (bad_alloc in a planner's vectors,
    // caught by the barrier at the end) or a failed builder frees it together with its sub-plans
    std::unique_ptr<cutensorPlan> pl(new (std::nothrow) cutensorPlan());
    if (pl == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    pl->kind = desc->kind;
    pl->dtype = desc->A.desc.dtype;
    pl->dtypeA = desc->A.desc.dtype;
    pl->dtypeB = desc->B.present ? desc->B.desc.dtype : desc->A.desc.dtype;
    if (desc->kind == OpKind::Contraction && pl->dtypeB != pl->dtypeA) pl->dtype = desc->D.desc.dtype;      // mixed fp64 x complex128: the output's
    pl->scalarType = desc->scalarType;
    pl->alignA = desc->A.desc.alignment;
    pl->alignB = desc->B.present ? desc->B.desc.alignment : 0;
    pl->alignC = desc->C.present ? desc->C.desc.alignment : 0;
    pl->alignD = desc->D.desc.alignment;
    pl->accumulate64 = accumulates_in_fp64(*desc);
    const cutensorStatus_t st = build_plan(PlanRequest{handle, *desc, pref, pr, workspaceSizeLimit}, *pl);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    if (memoable) memo_insert(handle, mkey, mhash, *pl);   // (only plans that own nothing a clone could not copy: plan_is_prototype)
    *plan = pl.release();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH


cutensorStatus_t cutensorDestroyPlan(cutensorPlan_t plan) try {
    delete plan;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction.cu:231-235
cutensorStatus_t cutensorPlanGetAttribute(const cutensorHandle_t handle, const cutensorPlan_t plan,
                                          cutensorPlanAttribute_t attr, void* buf, size_t sizeInBytes) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || buf == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (attr == CUTENSOR_PLAN_REQUIRED_WORKSPACE && sizeInBytes == sizeof(uint64_t)) {
        *static_cast<uint64_t*>(buf) = plan->requiredWorkspace;
        return CUTENSOR_STATUS_SUCCESS;
    }
    return CUTENSOR_STATUS_INVALID_VALUE;
} CTAMD_API_CATCH

// ---- execution -----------------------------------------------------------------------------------
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
    // incremental-autotuning trial: one event pair around everything this call launches, read later (resolve_pending_measurements)
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
            std::lock_guard<std::mutex> g(handle->mtx);
            handle->pending.push_back(cutensorHandle::PendingMeasurement{plan->tuneKey, plan->choice.kernel, plan->choice.splitK, t0, t1});
            handle->pendingCount.store((int)handle->pending.size(), std::memory_order_relaxed);
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

// contraction_jit.cu:134,398 — the engine has no run-time code generation (every kernel is compiled ahead of
// time for gfx950), so its "kernel cache" holds nothing: writing produces a small tagged file, reading checks
// the tag and reports IO_ERROR for a missing file exactly as the sample expects on its first run.
cutensorStatus_t cutensorWriteKernelCacheToFile(const cutensorHandle_t handle, const char filename[]) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (filename == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    FILE* f = std::fopen(filename, "w");
    if (f == nullptr) return CUTENSOR_STATUS_IO_ERROR;
    std::fprintf(f, "cutensor-amd-kernelcache 1 gfx950 0\n");
    std::fclose(f);
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH
cutensorStatus_t cutensorReadKernelCacheFromFile(cutensorHandle_t handle, const char filename[]) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (filename == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    FILE* f = std::fopen(filename, "r");
    if (f == nullptr) return CUTENSOR_STATUS_IO_ERROR;
    char tag[64] = {0};
    const bool ok = std::fscanf(f, "%63s", tag) == 1 && std::strcmp(tag, "cutensor-amd-kernelcache") == 0;
    std::fclose(f);
    return ok ? CUTENSOR_STATUS_SUCCESS : CUTENSOR_STATUS_IO_ERROR;
} CTAMD_API_CATCH

// utils.cuh:38
const char* cutensorGetErrorString(const cutensorStatus_t error) {
    switch (error) {
        case CUTENSOR_STATUS_SUCCESS: return "CUTENSOR_STATUS_SUCCESS";
        case CUTENSOR_STATUS_NOT_INITIALIZED: return "CUTENSOR_STATUS_NOT_INITIALIZED";
        case CUTENSOR_STATUS_ALLOC_FAILED: return "CUTENSOR_STATUS_ALLOC_FAILED";
        case CUTENSOR_STATUS_INVALID_VALUE: return "CUTENSOR_STATUS_INVALID_VALUE";
        case CUTENSOR_STATUS_ARCH_MISMATCH: return "CUTENSOR_STATUS_ARCH_MISMATCH";
        case CUTENSOR_STATUS_MAPPING_ERROR: return "CUTENSOR_STATUS_MAPPING_ERROR";
        case CUTENSOR_STATUS_EXECUTION_FAILED: return "CUTENSOR_STATUS_EXECUTION_FAILED";
        case CUTENSOR_STATUS_INTERNAL_ERROR: return "CUTENSOR_STATUS_INTERNAL_ERROR";
        case CUTENSOR_STATUS_NOT_SUPPORTED: return "CUTENSOR_STATUS_NOT_SUPPORTED";
        case CUTENSOR_STATUS_LICENSE_ERROR: return "CUTENSOR_STATUS_LICENSE_ERROR";
        case CUTENSOR_STATUS_CUBLAS_ERROR: return "CUTENSOR_STATUS_CUBLAS_ERROR";
        case CUTENSOR_STATUS_CUDA_ERROR: return "CUTENSOR_STATUS_CUDA_ERROR";
        case CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE: return "CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE";
        case CUTENSOR_STATUS_INSUFFICIENT_DRIVER: return "CUTENSOR_STATUS_INSUFFICIENT_DRIVER";
        case CUTENSOR_STATUS_IO_ERROR: return "CUTENSOR_STATUS_IO_ERROR";
        default: return "<unknown>";
    }
}

size_t cutensorGetVersion(void) { return CUTENSOR_VERSION; }

// ---- diagnostics (not part of the cuTENSOR ABI; used by the tests and the bench) ----------------
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

// cutensorContract launches by kernel kind since the library was loaded: out[0] gett_simple_kernel (scalar FMA fallback), [1]
// gett_wide_kernel (mode table), [2] fp32 MFMA families, [3] aligned 16-bit MFMA family, [4] general MFMA family.  Lets a test that
// drives the library through someone else's binding (the reference's own einsum.cc) assert which kernels its cases ran on.
int ctamdLastH16Kernel(void) try { return g_lastH16Kernel.load(std::memory_order_relaxed); } CTAMD_API_CATCH_INT

void ctamdLaunchCounts(uint64_t out[5]) try {
    for (int i = 0; i < 5; ++i) out[i] = g_launchCounts[i].load(std::memory_order_relaxed);
} CTAMD_API_CATCH_VOID

// Launches of the fp32 ring kernels that took the flat entry (kernels/gett_f32_stream.hip, launch_stream) since the library was loaded:
// tells a test which of the two entries its case ran on.
uint64_t ctamdFlatStartCount(void) try { return g_flatStartLaunches.load(std::memory_order_relaxed); } CTAMD_API_CATCH_ZERO

// Plan-memo counters of this handle: plans answered by cloning a prototype / plans that went through the planner.
void ctamdPlanMemoStats(const cutensorHandle_t handle, uint64_t* hits, uint64_t* misses, uint32_t* entries) try {
    if (handle == nullptr) return;
    if (hits) *hits = handle->memoHits.load(std::memory_order_relaxed);
    if (misses) *misses = handle->memoMisses.load(std::memory_order_relaxed);
    if (entries) { std::lock_guard<std::mutex> g(handle->mtx); *entries = (uint32_t)handle->planMemo.size(); }
} CTAMD_API_CATCH_VOID
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

// Instantiated fp32 GETT kernels (test coverage bookkeeping): table size, and whether entry i is a
// measurement-only ablation variant (never planned unless CUTENSOR_AMD_ABLATION is set).
// 1 when this library reads the test / measurement switches (CTAMD_HOOK_ENV: the lib_hooks/ flavour)
int ctamdTestHooksBuilt(void) try { return CTAMD_HOOKS_BUILT; } CTAMD_API_CATCH_INT

// CUTENSOR_LOG_LEVEL as this library read it: libcutensorMg.so logs its refusals under the same switch without reading it itself
int ctamdLogLevel(void) try { return log_level(); } CTAMD_API_CATCH_INT

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
