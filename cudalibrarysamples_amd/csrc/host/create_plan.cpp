// create_plan.cpp — cutensorCreatePlan: the plan memo in front, then one builder per plan kind (the routes of contraction_route.cpp decide,
// the builders here make the plan), the choice among a tiled contraction's ranked candidates (select_candidate: a trial of incremental
// autotuning, the plan cache's entry, the candidate the caller names, the measured one) and the two routines that measure on the device,
// autotune_contraction and calibrate_xcd_split.  The memo, the cache and the trial state live in the handle's PlanStore (plan_store.hpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>

#include <hip/hip_runtime.h>

#include "internal.hpp"

using namespace ctamd;

// A finished plan of the kinds plan_is_prototype lists becomes the prototype later plans of the same problem are cloned from
// (PlanStore::memo_insert).
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
static int autotune_contraction(const cutensorOperationDescriptor& op, const ContractionView& v, const std::vector<ContractionChoice>& ch) {
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
std::shared_ptr<const WideMode> ctamd::upload_mode_table(const std::vector<WideMode>& tab) {
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
    PlanStore& store = rq.handle->plans;
    const cutensorPlanPreference& pr = rq.pr;
    size_t idx = 0;
    // (a plan made under the "operands are streamed" preference neither reads nor feeds the per-problem cache: the cache is keyed by
    // the problem alone, and its entry belongs to the default policy.  A store of capacity 0 holds and answers nothing)
    const bool useCache = pr.cacheMode != CUTENSOR_CACHE_MODE_NONE && pr.operandsStreamed == 0;
    const bool explicitPick = names_candidate(pr);   // the caller names a candidate: the cache has no say
    const bool incremental = useCache && !explicitPick && pr.autotune == CUTENSOR_AUTOTUNE_MODE_INCREMENTAL;
    const bool patient = pr.algo == CUTENSOR_ALGO_DEFAULT_PATIENT;
    const bool needKey = incremental || (useCache && patient) || (useCache && !explicitPick && store.has_choices());
    const std::string key = needKey ? problem_key(rq.desc) : std::string();   // the string form is what the cache FILE holds
    // incremental autotuning (contraction_plan_cache.cu:215-237): the first INCREMENTAL_COUNT plans of a problem
    // are trials of candidates 0, 1, ... (timed by cutensorContract: the best of a trial plan's first few executions);
    // after that — and for every plan without the autotune mode — the cache answers with the fastest candidate
    // measured so far.  (The sample's loop is count + 1 rounds of which the last must hit the cache, :262.)
    if (incremental) {
        const int limit = std::min<int>(std::max<int32_t>(pr.incrementalCount, 1), (int)ch.size());
        if (const std::optional<int> rank = store.next_trial(key, limit)) {
            pl.tuneKey = key;
            return (size_t)*rank;
        }
    }
    if (needKey && useCache && !explicitPick)
        if (const std::optional<PlanStore::Choice> c = store.cached_choice(key))
            for (size_t i = 0; i < ch.size(); ++i)
                if (ch[i].kernel == c->kernel && ch[i].splitK == c->splitK) return i;
    if ((int)pr.algo >= 0) idx = std::min<size_t>((size_t)pr.algo, ch.size() - 1);
    else if (pr.kernelRank > 0) idx = std::min<size_t>((size_t)pr.kernelRank, ch.size() - 1);
    else if (patient) idx = (size_t)autotune_contraction(rq.desc, pl.view, ch);
    if (const char* f = CTAMD_HOOK_ENV("CUTENSOR_AMD_FORCE")) {   // "kernel:splitK" experiment knob
        int fk = -1; unsigned fs = 1;
        if (std::sscanf(f, "%d:%u", &fk, &fs) >= 1)
            for (size_t i = 0; i < ch.size(); ++i)
                if (ch[i].kernel == fk && ch[i].splitK == fs) { idx = i; break; }
    }
    // (a DEFAULT prototype memoised earlier must not shadow the measured choice: the store drops the memo with the write)
    if (useCache && patient) store.record_choice(key, ch[idx].kernel, ch[idx].splitK);
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
        std::string why;
        const cutensorStatus_t st = plan_elementwise_any(desc, rq.wsLimit, rq.handle->numCUs, pl.ew, pl.red, &why);
        if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreatePlan: %s", why.c_str()); return st; }
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
        std::string why;
        const cutensorStatus_t st = plan_elementwise_any(desc, rq.wsLimit, rq.handle->numCUs, pl.ew, pl.red, &why);
        if (st != CUTENSOR_STATUS_SUCCESS) { CT_LOG("cutensorCreatePlan: %s", why.c_str()); return st; }
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

extern "C" {

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
    PlanStore& store = handle->plans;
    PlanMemoKey mkey;
    uint64_t mhash = 0;
    bool memoable = pr.cacheMode != CUTENSOR_CACHE_MODE_NONE && !plan_env_override() && !(t_f64xOff > 0 && f64x_elem_of(*desc) >= 0) &&
                    build_memo_key(*desc, pr, workspaceSizeLimit, mkey);
    if (memoable) {
        mhash = mkey.hash();
        if (store.has_pending()) store.resolve();
        std::shared_ptr<const cutensorPlan> proto;
        switch (store.memo_lookup(mkey, mhash, proto)) {   // one lock: the capacity test, the lookup, the LRU stamp and the counters
            case PlanStore::Memo::Hit: {
                cutensorPlan* clone = clone_plan(*proto);
                if (clone == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
                *plan = clone;
                return CUTENSOR_STATUS_SUCCESS;
            }
            case PlanStore::Memo::Off: memoable = false; break;
            case PlanStore::Memo::Miss: break;
        }
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
    if (memoable && plan_is_prototype(*pl))   // (only plans that own nothing a clone could not copy)
        if (std::shared_ptr<const cutensorPlan> proto{clone_plan(*pl)}) store.memo_insert(mkey, mhash, std::move(proto));
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

}  // extern "C"
