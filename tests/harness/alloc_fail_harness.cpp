// alloc_fail_harness.cpp — "no exception crosses the C ABI" (csrc/host/api_guard.hpp), checked with a throwing operator new.
// The replaced global operator new of this executable is the one libcutensor.so's std::vector / std::map / std::string use (the
// library does not bind the symbol locally).  For k = 0, 1, 2, ... the k-th allocation of the call sequence of contraction.cu:123-235
// (handle, descriptors, contraction, preference, workspace estimate, plan, plan attribute) throws std::bad_alloc; every entry point
// must answer with a status — CUTENSOR_STATUS_ALLOC_FAILED — instead of letting the exception unwind into this C-style caller
// (std::terminate: the process would abort).  The sweep ends with the first k at which the whole sequence runs without a failure.
// No GPU needed: planning works on a handle without a device.
// The same operator new / delete count the live allocations: a round (one run of the sequence, with or without an injected failure) after
// which the count differs from before it left an object behind — an early return that forgot a `delete`, or an exception that unwound
// past a raw owner.  Every sweep prints the number of such rounds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>

#include <cutensor.h>
#include <cutensorMg.h>
#include <cutensorMp.h>

static long g_countdown = -1;   // < 0: never fail; otherwise the allocation that finds 0 here throws
static long g_thrown = 0;
static long g_live = 0;         // allocations made through operator new and not yet deleted

static void* guarded_alloc(std::size_t n) {
    if (g_countdown == 0) { g_countdown = -1; ++g_thrown; throw std::bad_alloc(); }
    if (g_countdown > 0) --g_countdown;
    void* p = std::malloc(n ? n : 1);
    if (p == nullptr) throw std::bad_alloc();
    ++g_live;
    return p;
}
static void guarded_free(void* p) noexcept { if (p != nullptr) { --g_live; std::free(p); } }
void* operator new(std::size_t n) { return guarded_alloc(n); }
void* operator new[](std::size_t n) { return guarded_alloc(n); }
void* operator new(std::size_t n, const std::nothrow_t&) noexcept { try { return guarded_alloc(n); } catch (...) { return nullptr; } }
void* operator new[](std::size_t n, const std::nothrow_t&) noexcept { try { return guarded_alloc(n); } catch (...) { return nullptr; } }
void operator delete(void* p) noexcept { guarded_free(p); }
void operator delete[](void* p) noexcept { guarded_free(p); }
void operator delete(void* p, std::size_t) noexcept { guarded_free(p); }
void operator delete[](void* p, std::size_t) noexcept { guarded_free(p); }

struct Outcome { int failed = 0, allocFailed = 0, other = 0; };

static bool ok(cutensorStatus_t s, Outcome& o) {
    if (s == CUTENSOR_STATUS_SUCCESS) return true;
    ++o.failed;
    if (s == CUTENSOR_STATUS_ALLOC_FAILED) ++o.allocFailed; else ++o.other;
    return false;
}

// the call sequence of contraction.cu:123-235 on a small problem; returns true when every call succeeded
static bool sequence(Outcome& o) {
    cutensorHandle_t h = nullptr;
    cutensorTensorDescriptor_t dA = nullptr, dB = nullptr, dC = nullptr;
    cutensorOperationDescriptor_t op = nullptr;
    cutensorPlanPreference_t pref = nullptr;
    cutensorPlan_t plan = nullptr;
    const int64_t eA[4] = {48, 16, 16, 48}, eB[4] = {32, 16, 32, 16}, eC[4] = {48, 32, 48, 32};
    const int32_t mA[4] = {'m', 'h', 'k', 'n'}, mB[4] = {'u', 'k', 'v', 'h'}, mC[4] = {'m', 'u', 'n', 'v'};
    bool good = ok(cutensorCreate(&h), o);
    good = good && ok(cutensorCreateTensorDescriptor(h, &dA, 4, eA, nullptr, HIP_R_32F, 128), o);
    good = good && ok(cutensorCreateTensorDescriptor(h, &dB, 4, eB, nullptr, HIP_R_32F, 128), o);
    good = good && ok(cutensorCreateTensorDescriptor(h, &dC, 4, eC, nullptr, HIP_R_32F, 128), o);
    good = good && ok(cutensorCreateContraction(h, &op, dA, mA, CUTENSOR_OP_IDENTITY, dB, mB, CUTENSOR_OP_IDENTITY, dC, mC,
                                                CUTENSOR_OP_IDENTITY, dC, mC, CUTENSOR_COMPUTE_DESC_32F), o);
    good = good && ok(cutensorCreatePlanPreference(h, &pref, CUTENSOR_ALGO_DEFAULT, CUTENSOR_JIT_MODE_NONE), o);
    uint64_t est = 0, req = 0;
    good = good && ok(cutensorEstimateWorkspaceSize(h, op, pref, CUTENSOR_WORKSPACE_DEFAULT, &est), o);
    good = good && ok(cutensorCreatePlan(h, &plan, op, pref, est), o);
    good = good && ok(cutensorPlanGetAttribute(h, plan, CUTENSOR_PLAN_REQUIRED_WORKSPACE, &req, sizeof(req)), o);
    // the destroy calls tolerate whatever was not created
    cutensorDestroyPlan(plan);
    cutensorDestroyPlanPreference(pref);
    cutensorDestroyOperationDescriptor(op);
    cutensorDestroyTensorDescriptor(dA);
    cutensorDestroyTensorDescriptor(dB);
    cutensorDestroyTensorDescriptor(dC);
    cutensorDestroy(h);
    return good;
}

// the call sequence of contraction_multi_gpu.cu:151-250 for C[i,j] = A[i,k] B[k,j] on two device ids (plan only: nothing executes)
static bool sequence_mg(Outcome& o) {
    cutensorMgHandle_t h = nullptr;
    cutensorMgTensorDescriptor_t dA = nullptr, dB = nullptr, dC = nullptr;
    cutensorMgContractionDescriptor_t con = nullptr;
    cutensorMgContractionFind_t find = nullptr;
    cutensorMgContractionPlan_t plan = nullptr;
    const int32_t devs[2] = {0, 1};
    const int64_t ext[2] = {256, 256}, blkRow[2] = {128, 256}, blkCol[2] = {256, 128}, blkC[2] = {128, 128};
    const int32_t cntRow[2] = {2, 1}, cntCol[2] = {1, 2};
    const int32_t mA[2] = {'i', 'k'}, mB[2] = {'k', 'j'}, mC[2] = {'i', 'j'};
    bool good = ok(cutensorMgCreate(&h, 2, devs), o);
    good = good && ok(cutensorMgCreateTensorDescriptor(h, &dA, 2, ext, nullptr, blkRow, nullptr, cntRow, 2, devs, HIP_R_32F), o);
    good = good && ok(cutensorMgCreateTensorDescriptor(h, &dB, 2, ext, nullptr, blkCol, nullptr, cntCol, 2, devs, HIP_R_32F), o);
    good = good && ok(cutensorMgCreateTensorDescriptor(h, &dC, 2, ext, nullptr, blkC, nullptr, cntRow, 2, devs, HIP_R_32F), o);
    good = good && ok(cutensorMgCreateContractionDescriptor(h, &con, dA, mA, dB, mB, dC, mC, dC, mC, CUTENSOR_COMPUTE_32F), o);
    good = good && ok(cutensorMgCreateContractionFind(h, &find, CUTENSORMG_ALGO_DEFAULT), o);
    int64_t devWs[2] = {0, 0}, hostWs = 0;
    good = good && ok(cutensorMgContractionGetWorkspace(h, con, find, CUTENSOR_WORKSPACE_DEFAULT, devWs, &hostWs), o);
    good = good && ok(cutensorMgCreateContractionPlan(h, &plan, con, find, devWs, hostWs), o);
    cutensorMgDestroyContractionPlan(plan);
    cutensorMgDestroyContractionFind(find);
    cutensorMgDestroyContractionDescriptor(con);
    cutensorMgDestroyTensorDescriptor(dA);
    cutensorMgDestroyTensorDescriptor(dB);
    cutensorMgDestroyTensorDescriptor(dC);
    cutensorMgDestroy(h);
    return good;
}

// The cuTENSORMp planning sequence of cutensorMp_contraction.cu:473-509 on rank 1 of a local world (plan only).  The world and the handle
// are made once, before the sweep: a handle is per process and rank, the calls below are per contraction.
static void* g_world = nullptr;
static cutensorMpHandle_t g_mp = nullptr;
struct MpLayout { int64_t ext[3]; int64_t pA[2], pB[2], pC[2]; int64_t pad; };   // extents m, k, n; ranks per mode; first-mode padding of C
static bool sequence_mp_layout(Outcome& o, const MpLayout& L) {
    cutensorMpTensorDescriptor_t dA = nullptr, dB = nullptr, dC = nullptr;
    cutensorMpOperationDescriptor_t op = nullptr;
    cutensorMpPlanPreference_t pref = nullptr;
    cutensorMpPlan_t plan = nullptr;
    const int64_t eA[2] = {L.ext[0], L.ext[1]}, eB[2] = {L.ext[1], L.ext[2]}, eC[2] = {L.ext[0], L.ext[2]};
    const int64_t sC[2] = {1, (L.ext[0] + L.pC[0] - 1) / L.pC[0] + L.pad};
    const int32_t mA[2] = {'m', 'k'}, mB[2] = {'k', 'n'}, mC[2] = {'m', 'n'};
    bool good = ok(cutensorMpCreateTensorDescriptor(g_mp, &dA, 2, eA, nullptr, nullptr, nullptr, L.pA, 4, nullptr, HIP_R_32F), o);
    good = good && ok(cutensorMpCreateTensorDescriptor(g_mp, &dB, 2, eB, nullptr, nullptr, nullptr, L.pB, 4, nullptr, HIP_R_32F), o);
    good = good && ok(cutensorMpCreateTensorDescriptor(g_mp, &dC, 2, eC, L.pad ? sC : nullptr, nullptr, nullptr, L.pC, 4, nullptr, HIP_R_32F), o);
    good = good && ok(cutensorMpCreateContraction(g_mp, &op, dA, mA, CUTENSOR_OP_IDENTITY, dB, mB, CUTENSOR_OP_IDENTITY, dC, mC,
                                                  CUTENSOR_OP_IDENTITY, dC, mC, CUTENSOR_COMPUTE_DESC_32F), o);
    good = good && ok(cutensorMpCreatePlanPreference(g_mp, &pref, CUTENSORMP_ALGO_DEFAULT, 1ull << 30, 0), o);
    good = good && ok(cutensorMpCreatePlan(g_mp, &plan, op, pref), o);
    uint64_t req = 0;
    good = good && ok(cutensorMpPlanGetAttribute(g_mp, plan, CUTENSORMP_PLAN_REQUIRED_WORKSPACE_DEVICE, &req, sizeof(req)), o);
    char text[256];
    if (good && ctamdMpDescribePlan(plan, text, sizeof text) == 0) { ++o.failed; ++o.allocFailed; good = false; }   // 0: the description ran out of memory
    cutensorMpDestroyPlan(plan);
    cutensorMpDestroyPlanPreference(pref);
    cutensorMpDestroyOperationDescriptor(op);
    cutensorMpDestroyTensorDescriptor(dA);
    cutensorMpDestroyTensorDescriptor(dB);
    cutensorMpDestroyTensorDescriptor(dC);
    return good;
}
// gather: mk,kn->mn, extents 64, A cut 4-way along k, B 4-way along n, C on a 2 x 2 grid (sub-box transfers, staging, unpack copies)
static bool sequence_mp_gather(Outcome& o) { return sequence_mp_layout(o, MpLayout{{64, 64, 64}, {1, 4}, {1, 4}, {2, 2}, 0}); }
// reduce (the byte counts choose it: |C| is small against the operands): A and B cut 4-way along k, C cut 4-way along m with padded element
// strides — the partial is staged, the destination blocks are packed into slots and the received slot is unpacked (cIn, pack, unpack exist)
static bool sequence_mp_reduce(Outcome& o) { return sequence_mp_layout(o, MpLayout{{24, 256, 16}, {1, 4}, {4, 1}, {4, 1}, 3}); }

static int sweep(const char* what, bool (*seq)(Outcome&)) {
    Outcome warm;
    if (!seq(warm)) { std::printf("%s: the sequence fails without any injected failure\n", what); return 2; }
    long injected = 0, answered = 0, leaky = 0;
    for (long k = 0; k < 100000; ++k) {
        Outcome o;
        const long before = g_thrown, liveBefore = g_live;
        g_countdown = k;
        const bool good = seq(o);
        g_countdown = -1;
        if (g_live != liveBefore) ++leaky;
        if (g_thrown == before) {            // the sequence needs fewer than k allocations: the sweep is complete
            if (!good) { std::printf("%s: k = %ld: failure without an injected bad_alloc\n", what, k); return 3; }
            std::printf("%s: alloc guard ok: %ld injected failures, %ld answered with a status\n", what, injected, answered);
            std::printf("%s: %ld rounds left allocations behind\n", what, leaky);
            return injected > 0 && answered > 0 ? 0 : 4;
        }
        ++injected;
        if (!good) {
            ++answered;
            if (o.other != 0) { std::printf("%s: k = %ld: a status other than ALLOC_FAILED\n", what, k); return 5; }
        }
        // (good && thrown: the failure hit a nothrow allocation or an optional path the library recovers from)
    }
    std::printf("%s: the sweep did not terminate\n", what);
    return 6;
}

// the three tensor-descriptor calls of `sequence` alone (the handle is made outside the sweep)
static cutensorHandle_t g_engine = nullptr;
static bool sequence_descriptors(Outcome& o) {
    cutensorTensorDescriptor_t d[3] = {nullptr, nullptr, nullptr};
    const int64_t e[4] = {48, 16, 16, 48}, s[4] = {1, 50, 800, 12800};
    bool good = ok(cutensorCreateTensorDescriptor(g_engine, &d[0], 4, e, nullptr, HIP_R_32F, 128), o);
    good = good && ok(cutensorCreateTensorDescriptor(g_engine, &d[1], 4, e, s, HIP_R_32F, 128), o);
    good = good && ok(cutensorCreateTensorDescriptor(g_engine, &d[2], 1, e, nullptr, HIP_R_64F, 8), o);
    for (auto x : d) cutensorDestroyTensorDescriptor(x);
    return good;
}

static int sweep_mp() {
    if (ctamdMpLocalWorldCreate(&g_world, 4) != CUTENSOR_STATUS_SUCCESS) return 7;
    if (ctamdMpCreateOnLocalWorld(&g_mp, g_world, 1, 0, nullptr) != CUTENSOR_STATUS_SUCCESS) return 7;
    int rc = sweep("cutensorMp gather", sequence_mp_gather);
    if (rc == 0) rc = sweep("cutensorMp reduce", sequence_mp_reduce);
    if (rc == 0) std::printf("cutensorMp: alloc guard ok\n");
    cutensorMpDestroy(g_mp);
    ctamdMpLocalWorldDestroy(g_world);
    return rc;
}

int main(int argc, char** argv) {
    int rc = sweep("cutensor", sequence);
    if (rc == 0 && cutensorCreate(&g_engine) == CUTENSOR_STATUS_SUCCESS) {
        rc = sweep("cutensor descriptors", sequence_descriptors);
        cutensorDestroy(g_engine);
    }
    if (rc == 0 && argc > 1 && argv[1][0] == 'm') rc = sweep("cutensorMg", sequence_mg);
    if (rc == 0 && argc > 1 && argv[1][0] == 'm') rc = sweep_mp();
    return rc;
}
