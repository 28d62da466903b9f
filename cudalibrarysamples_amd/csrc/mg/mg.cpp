// mg.cpp — cuTENSORMg on a node of MI355X GPUs: single process, one host thread, N devices.
//
// Serves the call sequence of cuTENSORMg/contraction_multi_gpu.cu (create handle :151, block-cyclic
// tensor descriptors :195-217, contraction descriptor / find / workspace / plan :228-250,
// cutensorMgContraction :328-332) and of cuTENSORMg/blog_post.cu (:131-145, :286-302).  Built entirely
// on the public single-GPU ABI (include/cutensor.h), HIP and RCCL.
//
// Algorithm ("shard the largest free mode, gather the rest, overlap the gather with the first pieces"):
//   1. The largest free mode p of C (carried by exactly one operand X) is cut into one contiguous shard
//      per handle device; shards are cut again at p's block boundaries so that every piece lies in one block.
//   2. The other operand Y does not carry p: every device needs all of it (an all-gather).  When Y is
//      distributed along a free mode q, the device's work is cut along q's grid coordinate as well: the
//      coordinates whose cells the device already holds come first (no remote dependency), the remote ones
//      follow in contiguous runs, so the first local contraction starts while the gather is in flight.
//   3. An operand view that touches a single grid cell living on the computing device is read (or, for D,
//      written) in place.  Everything else is staged in the device's workspace as an image [cell][cell
//      buffer]: local cells by device copies on the device's own stream, remote cells over xGMI by RCCL
//      ncclSend / ncclRecv pairs inside ONE ncclGroup per wave on a separate communication stream per
//      device (or by peer copies on several streams: CUTENSORMG_AMD_TRANSPORT=peer, and when RCCL is not
//      available).  Every wave records an event; a piece waits only for the waves that carry its cells.
//   4. The staged image *is* a tensor: mode i becomes (w_i inside a block, block-index digits) with strides
//      (elementStride_i, cellElems * cellStride_i per grid digit, blockStride_i per local-block digit); the
//      local contraction is one cutensorContract per piece on these strided views — no redistribution kernel.
//   5. Pieces alternate between the caller's stream and an auxiliary stream per device (two local
//      contractions in flight hide each other's tails); staged pieces of C are copied to the owners' cells
//      by identity cutensorPermute on strided views (peer stores over xGMI when the owner is remote).
//
// Shared modes must have the same block size in every tensor that carries them; their device counts may
// differ when they divide each other (e.g. B distributed along j, C not): the block index is then split
// into common mixed-radix digits.  A tensor in any other layout is brought into an accepted one by cutensorMgCopy
// (mg_copy.cpp).
//
// Files of csrc/mg: mg.cpp (this one: handle and descriptor entry points, and the two contraction entry points as the sequence of their
// steps), mg_internal.hpp (shared structs, the event-block layout, walk_piece), mg_workers.h (worker threads), mg_views.cpp (index
// arithmetic of the views), mg_contraction_plan.cpp (steps of the plan builder), mg_contraction_exec.cpp (phases of a call),
// mg_diagnostics.cpp (descriptions, host replay), mg_copy.cpp (cutensorMgCopy), mg_kernels.hip / mg_redistribute.hip (kernels).
#include <algorithm>
#include <new>
#include <set>

#include "mg_internal.hpp"

using namespace ctamd_mg;

extern "C" {

// contraction_multi_gpu.cu:151
cutensorStatus_t cutensorMgCreate(cutensorMgHandle_t* handle, uint32_t numDevices, const int32_t devices[]) try {
    if (handle == nullptr || numDevices == 0 || devices == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    DeviceGuard guard;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    cutensorMgHandle* h = new (std::nothrow) cutensorMgHandle();
    if (h == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    h->haveDevice = count > 0;
    h->devices.assign(devices, devices + numDevices);
    std::set<int32_t> uniq(h->devices.begin(), h->devices.end());
    h->distinct = uniq.size() == h->devices.size();
    h->forceGather = env_is("CUTENSORMG_AMD_FORCE_GATHER", "1");
    for (int32_t d : h->devices) {
        if (d < 0 || (count > 0 && d >= count)) { cutensorMgDestroy(h); return CUTENSOR_STATUS_INVALID_VALUE; }
        if (count > 0) (void)hipSetDevice(d);
        cutensorHandle_t ch = nullptr;
        if (cutensorCreate(&ch) != CUTENSOR_STATUS_SUCCESS) { cutensorMgDestroy(h); return CUTENSOR_STATUS_ALLOC_FAILED; }
        h->handles.push_back(ch);
        if (count > 0)
            for (int32_t o : uniq)
                if (o != d) { (void)hipDeviceEnablePeerAccess(o, 0); (void)hipGetLastError(); }   // xGMI peer mapping
    }
    if (count > 0 && h->distinct && (numDevices > 1 || h->forceGather) && !env_is("CUTENSORMG_AMD_TRANSPORT", "peer")) {
        h->comms.resize(numDevices);
        std::vector<int> devs(h->devices.begin(), h->devices.end());
        if (ncclCommInitAll(h->comms.data(), (int)numDevices, devs.data()) != ncclSuccess) h->comms.clear();
    }
    // worker threads for the per-device parts of a call (MgWorkers): from FOUR handle devices on — measured (tools/mg_host_cost_n.py, bench
    // layout, us per call idle / back to back, workers against one thread): two devices 21 / 15 against 14 / 14, four 28 / 20 against
    // 23 / 26, eight 35 / 27.5 against 47 / 48 (profiles/r06r_mg_host_cost_*).  CUTENSORMG_AMD_THREADS (hooks flavour): 0 keeps
    // everything on the calling thread, 1 starts the workers from two devices on
    const bool wantWorkers = CTAMD_HOOK_IS("CUTENSORMG_AMD_THREADS", "1") ? numDevices > 1 : (numDevices >= 4 && !CTAMD_HOOK_IS("CUTENSORMG_AMD_THREADS", "0"));
    if (count > 0 && wantWorkers) h->workers.start((int)numDevices, [devs = h->devices](int g) { (void)hipSetDevice(devs[(size_t)g]); });
    *handle = h;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:383
cutensorStatus_t cutensorMgDestroy(cutensorMgHandle_t handle) try {
    if (handle == nullptr) return CUTENSOR_STATUS_SUCCESS;
    DeviceGuard guard;
    for (size_t g = 0; g < handle->commStreams.size(); ++g) {
        if (handle->haveDevice) (void)hipSetDevice(handle->devices[g]);
        for (hipStream_t s : handle->commStreams[g]) (void)hipStreamDestroy(s);
        if (g < handle->auxStreams.size() && handle->auxStreams[g]) (void)hipStreamDestroy(handle->auxStreams[g]);
    }
    handle->workers.shutdown();
    for (ncclComm_t c : handle->comms) (void)ncclCommDestroy(c);
    for (cutensorHandle_t h : handle->handles) cutensorDestroy(h);
    delete handle;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:195-197
cutensorStatus_t cutensorMgCreateTensorDescriptor(const cutensorMgHandle_t handle, cutensorMgTensorDescriptor_t* desc,
                                                  uint32_t numModes, const int64_t extent[], const int64_t elementStride[],
                                                  const int64_t blockSize[], const int64_t blockStride[],
                                                  const int32_t deviceCount[], uint32_t numDevices, const int32_t devices[],
                                                  cudaDataType_t type) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || (numModes > 0 && extent == nullptr) || devices == nullptr || numDevices == 0) return CUTENSOR_STATUS_INVALID_VALUE;
    if (numModes > 20 || elem_size(type) == 0) return CUTENSOR_STATUS_NOT_SUPPORTED;
    cutensorMgTensorDescriptor* d = new (std::nothrow) cutensorMgTensorDescriptor();
    if (d == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    MgTensor& t = d->t;
    t.n = numModes;
    t.dtype = type;
    t.extent.assign(extent, extent + numModes);
    t.blockSize.resize(numModes); t.deviceCount.resize(numModes); t.localBlocks.resize(numModes);
    t.elemStride.resize(numModes); t.blockStride.resize(numModes); t.cellStride.resize(numModes);
    int64_t cells = 1, run = 1;
    for (uint32_t i = 0; i < numModes; ++i) {
        if (extent[i] <= 0) { delete d; return CUTENSOR_STATUS_INVALID_VALUE; }
        t.blockSize[i] = blockSize ? blockSize[i] : extent[i];
        t.deviceCount[i] = deviceCount ? deviceCount[i] : 1;
        if (t.blockSize[i] <= 0 || t.deviceCount[i] <= 0) { delete d; return CUTENSOR_STATUS_INVALID_VALUE; }
        // every cell stores whole blocks: ceil(ceil(extent / blockSize) / deviceCount) of them per mode, exactly what the
        // samples allocate (contraction_multi_gpu.cu:256 discretize(); blog_post.cu:107-113).  A ragged extent leaves
        // padding at the end of the index space; the contraction descriptor decides whether that is acceptable.
        const int64_t blocks = (extent[i] + t.blockSize[i] - 1) / t.blockSize[i];
        t.localBlocks[i] = (blocks + t.deviceCount[i] - 1) / t.deviceCount[i];
        t.cellStride[i] = cells;
        cells *= t.deviceCount[i];
        t.elemStride[i] = elementStride ? elementStride[i] : run;
        run *= t.blockSize[i];
    }
    int64_t brun = run;   // packed block stride: one whole block, then blocks of mode 0, 1, ...
    for (uint32_t i = 0; i < numModes; ++i) {
        t.blockStride[i] = blockStride ? blockStride[i] : brun;
        brun *= t.localBlocks[i];
    }
    if ((int64_t)numDevices != cells) { delete d; return CUTENSOR_STATUS_INVALID_VALUE; }
    for (uint32_t i = 0; i < numDevices; ++i)
        if (devices[i] == CUTENSOR_MG_DEVICE_HOST) { delete d; return CUTENSOR_STATUS_NOT_SUPPORTED; }
    t.devices.assign(devices, devices + numDevices);
    t.numCells = cells;
    int64_t span = 1;
    for (uint32_t i = 0; i < numModes; ++i)
        span += (t.blockSize[i] - 1) * t.elemStride[i] + (t.localBlocks[i] - 1) * t.blockStride[i];
    t.cellElems = span;
    *desc = d;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyTensorDescriptor(cutensorMgTensorDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:228-233
cutensorStatus_t cutensorMgCreateContractionDescriptor(const cutensorMgHandle_t handle, cutensorMgContractionDescriptor_t* desc,
                                                       const cutensorMgTensorDescriptor_t descA, const int32_t modesA[],
                                                       const cutensorMgTensorDescriptor_t descB, const int32_t modesB[],
                                                       const cutensorMgTensorDescriptor_t descC, const int32_t modesC[],
                                                       const cutensorMgTensorDescriptor_t descD, const int32_t modesD[],
                                                       cutensorComputeType_t compute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || descA == nullptr || descB == nullptr || descC == nullptr || descD == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorMgContractionDescriptor* d = new (std::nothrow) cutensorMgContractionDescriptor();
    if (d == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    d->A = descA->t; d->B = descB->t; d->C = descC->t; d->D = descD->t;
    d->mA.assign(modesA, modesA + d->A.n);
    d->mB.assign(modesB, modesB + d->B.n);
    d->mC.assign(modesC, modesC + d->C.n);
    std::vector<int32_t> mD(modesD, modesD + d->D.n);
    d->compute = compute;
    // D must be distributed exactly like C (the sample passes the same descriptor twice)
    const bool sameCD = mD == d->mC && d->C.extent == d->D.extent && d->C.blockSize == d->D.blockSize &&
                        d->C.deviceCount == d->D.deviceCount && d->C.elemStride == d->D.elemStride &&
                        d->C.blockStride == d->D.blockStride && d->C.devices == d->D.devices;
    if (!sameCD || d->A.dtype != d->B.dtype || d->A.dtype != d->C.dtype) { delete d; return CUTENSOR_STATUS_NOT_SUPPORTED; }
    // a mode shared by two tensors must be cut into the same blocks in both, and the two device counts must divide one
    // another (the block index then has common mixed-radix digits)
    auto check = [&](const MgTensor& x, const std::vector<int32_t>& mx, const MgTensor& y, const std::vector<int32_t>& my) {
        for (uint32_t i = 0; i < x.n; ++i) {
            const int j = find_label(my, mx[i]);
            if (j < 0) continue;
            if (x.extent[i] != y.extent[j]) return CUTENSOR_STATUS_INVALID_VALUE;
            if (x.blockSize[i] != y.blockSize[j]) return CUTENSOR_STATUS_NOT_SUPPORTED;
            const int64_t a = x.deviceCount[i], b = y.deviceCount[j];
            if (a % b != 0 && b % a != 0) return CUTENSOR_STATUS_NOT_SUPPORTED;
            if (x.localBlocks[i] * a != y.localBlocks[j] * b) return CUTENSOR_STATUS_NOT_SUPPORTED;   // same padded block count
        }
        return CUTENSOR_STATUS_SUCCESS;
    };
    cutensorStatus_t st = check(d->A, d->mA, d->B, d->mB);
    if (st == CUTENSOR_STATUS_SUCCESS) st = check(d->A, d->mA, d->C, d->mC);
    if (st == CUTENSOR_STATUS_SUCCESS) st = check(d->B, d->mB, d->C, d->mC);
    // Ragged extents (not a multiple of blockSize * deviceCount; blog_post.cu:168-175 derives every block size with ceil()):
    // a ragged mode of C only produces extra results in the padding of D's cells, which the caller never reads, so the local
    // contractions simply run over the padded index space; a ragged CONTRACTED mode would put the padding into every sum, so
    // the plan clips it: the valid part of its index space is tiled by boxes (kbox_list) that accumulate into D.
    if (st != CUTENSOR_STATUS_SUCCESS) { delete d; return st; }
    *desc = d;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyContractionDescriptor(cutensorMgContractionDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:236-237
cutensorStatus_t cutensorMgCreateContractionFind(const cutensorMgHandle_t handle, cutensorMgContractionFind_t* find,
                                                 const cutensorMgAlgo_t algo) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (find == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorMgContractionFind* f = new (std::nothrow) cutensorMgContractionFind();
    if (f == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    f->algo = algo;
    *find = f;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyContractionFind(cutensorMgContractionFind_t find) try {
    delete find;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:241-242
cutensorStatus_t cutensorMgContractionGetWorkspace(const cutensorMgHandle_t handle, const cutensorMgContractionDescriptor_t desc,
                                                   const cutensorMgContractionFind_t find, cutensorWorksizePreference_t preference,
                                                   int64_t deviceWorkspaceSize[], int64_t* hostWorkspaceSize) try {
    (void)find; (void)preference;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || deviceWorkspaceSize == nullptr || hostWorkspaceSize == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    int64_t s[3];
    staging_sizes(*desc, s);
    for (size_t i = 0; i < handle->devices.size(); ++i)
        deviceWorkspaceSize[i] = s[0] + s[1] + s[2] + (int64_t)(kComputeStreams * kLocalContractionWs);
    *hostWorkspaceSize = 0;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:249-250 — the steps are in mg_contraction_plan.cpp
cutensorStatus_t cutensorMgCreateContractionPlan(const cutensorMgHandle_t handle, cutensorMgContractionPlan_t* plan,
                                                 const cutensorMgContractionDescriptor_t desc, const cutensorMgContractionFind_t find,
                                                 const int64_t deviceWorkspaceSize[], int64_t hostWorkspaceSize) try {
    (void)find; (void)hostWorkspaceSize;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || desc == nullptr || deviceWorkspaceSize == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    DeviceGuard guard;
    PlanPtr pl(new (std::nothrow) cutensorMgContractionPlan());      // released with whatever it holds on every exit but the last
    if (pl == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    pl->desc = *desc;
    pl->owner = handle;
    const int nDev = (int)handle->devices.size();
    const PlanInputs in{handle, pl->desc, Operands(pl->desc), nDev, elem_size(pl->desc.A.dtype), waves_wanted()};
    // the workspace: the staging images, and what is left of it for the local contractions of the two compute streams
    staging_sizes(pl->desc, pl->stagingBytes);
    const int64_t fixed = pl->stagingBytes[0] + pl->stagingBytes[1] + pl->stagingBytes[2];
    pl->contractionWs = kLocalContractionWs;
    for (int g = 0; g < nDev; ++g) {
        if (deviceWorkspaceSize[g] < fixed) return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
        pl->contractionWs = std::min<uint64_t>(pl->contractionWs, (uint64_t)(deviceWorkspaceSize[g] - fixed) / kComputeStreams / 256 * 256);
    }
    pl->forceGather = handle->forceGather;
    pl->useRccl = !handle->comms.empty() ||
                  // plan-only handles (no GPU visible): CPU tests of the RCCL event wiring and transport choice
                  (!handle->haveDevice && handle->distinct && (nDev > 1 || handle->forceGather) && CTAMD_HOOK_IS("CUTENSORMG_AMD_ASSUME_RCCL", "1"));

    Labels lab;
    cutensorStatus_t st = build_radix(in, &lab);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    const Sharding sh = choose_sharding(in, lab);
    pl->pLabel = sh.pC >= 0 ? pl->desc.mC[sh.pC] : -1;
    pl->p2Label = sh.p2C >= 0 ? pl->desc.mC[sh.p2C] : -1;
    pl->qLabel = sh.qLi >= 0 ? lab.universe[sh.qLi] : -1;
    pl->pieces = cut_pieces(in, lab, sh);
    plan_transfers(in, lab, sh, pl.get());
    classify_transport(in, pl.get());
    Boxes boxes;
    st = contracted_boxes(in, lab, &boxes);
    pl->numBoxes = (int)boxes.size();
    for (Piece& p : pl->pieces) {
        if (st == CUTENSOR_STATUS_SUCCESS) st = build_local_plans(in, lab, sh, boxes, p, pl.get());
        if (st == CUTENSOR_STATUS_SUCCESS) st = build_scatter_plans(in, lab, sh, p);
    }
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    scatter_owners(in, pl.get());
    *plan = pl.release();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyContractionPlan(cutensorMgContractionPlan_t plan) try {
    PlanDeleter()(plan);
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:328-332 — the phases are in mg_contraction_exec.cpp
cutensorStatus_t cutensorMgContraction(const cutensorMgHandle_t handle, const cutensorMgContractionPlan_t plan,
                                       const void* alpha, const void* A[], const void* B[], const void* beta,
                                       const void* C[], void* D[], void* workspaceDevice[], void* workspaceHost,
                                       cudaStream_t streams[]) try {
    (void)workspaceHost;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || alpha == nullptr || beta == nullptr || A == nullptr || B == nullptr || D == nullptr ||
        workspaceDevice == nullptr || streams == nullptr)
        return CUTENSOR_STATUS_INVALID_VALUE;
    if (!handle->haveDevice) return CUTENSOR_STATUS_ARCH_MISMATCH;   // plan-only handle (no GPU visible)
    DeviceGuard guard;
    const MgCall call(handle, plan, alpha, A, B, beta, C, D, workspaceDevice, streams);
    if (!call.betaIsZero && C == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (!ensure_runtime(handle, plan)) { (void)hipGetLastError(); return CUTENSOR_STATUS_EXECUTION_FAILED; }
    const int numWaves = plan->ev.numWaves;

    cutensorStatus_t st = fork(call);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    WorkerPhases workers(call);      // from here on, per-device phases go to the handle's worker threads when it has them
    // a call without remote cells has nothing for this thread to do in between: the workers run staging and pieces in ONE phase
    const bool onePhase = call.threaded && numWaves == 0 && !call.anyComm;
    if (!onePhase) st = workers.begin({stage_local});            // workers: returns at once, this thread goes on with the remote cells
    Transport transport;
    if (st == CUTENSOR_STATUS_SUCCESS) st = choose_transport(call, &transport);
    for (int w = 0; w < numWaves && st == CUTENSOR_STATUS_SUCCESS; ++w) st = gather_wave(call, w, transport);
    if (st == CUTENSOR_STATUS_SUCCESS && numWaves == 0) st = end_trial(call, transport);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    st = workers.collect();          // the staging copies are queued: the pieces of a device follow them on the same worker
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    st = onePhase ? workers.run({stage_local, run_pieces, join_own}) : workers.run({run_pieces, join_own});
    if (st == CUTENSOR_STATUS_SUCCESS && any_cross_join(call)) st = workers.run({join_cross});
    return st;
} CTAMD_API_CATCH

}  // extern "C"
