// mp.cpp — cuTENSORMp on MI355X: one process per GPU, RCCL point-to-point exchange over xGMI.
//
// Serves the call sequence of cutensorMp/cutensorMp_contraction.cu (handle :470-471, distributed tensor
// descriptors :473-483, contraction / preference / plan :485-509, cutensorMpContract :537-538).  Built on the
// public single-GPU ABI (include/cutensor.h), HIP and RCCL.
//
// Algorithm ("owner computes, gather what you need"):
//   1. Rank r owns one block ("cell") of C / D.  Its range in every mode of C fixes the box of A and of B it needs:
//      the same range in the modes an operand shares with C, the full extent in the contracted modes.
//   2. Every rank intersects that box with the cells of A and B.  A non-empty intersection is one transfer
//      owner -> r of exactly that sub-box: the owner packs it (a strided identity cutensorPermute) unless it is its
//      whole contiguous block, all transfers of a call travel in ONE ncclGroup of send/recv pairs, and the receiver
//      unpacks into a dense staging tensor.  Both sides derive the same transfer list from the descriptors, so no
//      metadata is exchanged.  An operand whose needed box lies inside the rank's own block is used in place.
//   3. One cutensorContract per rank: staged (or in-place) views of A and B, D written straight into the rank's
//      own block — the result needs no scatter and beta * C needs no exchange.
// The local contraction therefore always sees dense, packed operands (the GETT engine's fast layouts); the price
// is that a contracted mode distributed over ranks is gathered rather than reduced.
//
// Second algorithm ("stationary inputs, reduce the result") for the opposite shape — A and B distributed identically
// along contracted modes only, e.g. the headline einsum with K cut over the ranks: every rank contracts its own K
// slice in place (no operand moves at all) into a full-size partial of C, and ONE RCCL collective finishes the job:
// ncclAllReduce when C is replicated, ncclReduceScatter (destination blocks packed into equal slots) when C is
// distributed.  beta * C enters the sum exactly once (rank 0 for a replicated C, the owner's block otherwise).
// Every rank picks the algorithm from the same global byte counts, so the choice needs no communication.
//
// The files of the library: mp_internal.hpp.  This one holds the handle, descriptor and preference entry points, and
// cutensorMpCreatePlan / cutensorMpContract as argument checks plus the sequence of their steps (mp_plan.cpp, mp_call.cpp).
#include <memory>
#include <new>
#include <vector>

#include "mp_internal.hpp"

using namespace ctamd_mp;

extern "C" {

// Makes localDevice current for the creation of the single-GPU handle and hands the Mp handle out.
static cutensorStatus_t finish_handle(std::unique_ptr<cutensorMpHandle> h, int localDevice, hipStream_t stream, cutensorMpHandle_t* out) {
    h->device = localDevice;
    h->stream = stream;
    DeviceGuard guard;
    if (hipSetDevice(localDevice) != hipSuccess) {
        (void)hipGetLastError();
        int count = 0;
        const bool noGpu = hipGetDeviceCount(&count) != hipSuccess || count == 0;
        (void)hipGetLastError();
        // a machine without any GPU can still build and inspect plans (the planner of the single-GPU library works there
        // too); execution fails in the first HIP call.  A wrong device index on a machine with GPUs is an error.
        if (!noGpu) return CUTENSOR_STATUS_INVALID_VALUE;
        h->device = -1;
    }
    const cutensorStatus_t st = cutensorCreate(&h->h);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    h->transport->set_engine(h->h);
    *out = h.release();
    return CUTENSOR_STATUS_SUCCESS;
}

// cutensorMp_contraction.cu:470-471
cutensorStatus_t cutensorMpCreate(cutensorMpHandle_t* handle, ncclComm_t comm, int localDevice, cudaStream_t stream) try {
    if (handle == nullptr || comm == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    int rank = 0, n = 0;
    if (!rccl_rank_and_size(comm, &rank, &n)) return CUTENSOR_STATUS_INVALID_VALUE;
    std::unique_ptr<cutensorMpHandle> h(new (std::nothrow) cutensorMpHandle());
    if (h == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    h->transport.reset(new_rccl_transport(comm, rank, n));
    if (h->transport == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    return finish_handle(std::move(h), localDevice, stream, handle);
} CTAMD_API_CATCH

cutensorStatus_t cutensorMpDestroy(cutensorMpHandle_t handle) try {
    delete handle;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t ctamdMpLocalWorldCreate(void** world, int nranks) try {
    if (world == nullptr || nranks <= 0) return CUTENSOR_STATUS_INVALID_VALUE;
    LocalWorld* w = new_local_world(nranks);
    if (w == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    *world = w;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH
cutensorStatus_t ctamdMpLocalWorldDestroy(void* world) try {
    delete_local_world(static_cast<LocalWorld*>(world));
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH
cutensorStatus_t ctamdMpCreateOnLocalWorld(cutensorMpHandle_t* handle, void* world, int rank, int localDevice, cudaStream_t stream) try {
    LocalWorld* w = static_cast<LocalWorld*>(world);
    if (handle == nullptr || w == nullptr || rank < 0 || rank >= local_world_size(w)) return CUTENSOR_STATUS_INVALID_VALUE;
    std::unique_ptr<cutensorMpHandle> h(new (std::nothrow) cutensorMpHandle());
    if (h == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    h->transport.reset(new_local_transport(w, rank));
    if (h->transport == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    return finish_handle(std::move(h), localDevice, stream, handle);
} CTAMD_API_CATCH

// cutensorMp_contraction.cu:474-483
cutensorStatus_t cutensorMpCreateTensorDescriptor(const cutensorMpHandle_t handle, cutensorMpTensorDescriptor_t* desc,
                                                  uint32_t numModes, const int64_t extent[], const int64_t elementStride[],
                                                  const int64_t blockSize[], const int64_t blockStride[],
                                                  const int64_t nranksPerMode[], uint32_t nranks, const int32_t ranks[],
                                                  cutensorDataType_t type) try {
    (void)blockStride;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || (numModes > 0 && extent == nullptr)) return CUTENSOR_STATUS_INVALID_VALUE;
    if (numModes > 62 || elem_size(type) == 0) return CUTENSOR_STATUS_NOT_SUPPORTED;
    std::unique_ptr<cutensorMpTensorDescriptor> d(new (std::nothrow) cutensorMpTensorDescriptor());
    if (d == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    MpTensor& t = d->t;
    t.n = numModes;
    t.dtype = type;
    t.extent.assign(extent, extent + numModes);
    t.p.resize(numModes); t.bs.resize(numModes); t.elemStride.resize(numModes); t.cellStride.resize(numModes);
    int64_t cells = 1, run = 1;
    for (uint32_t i = 0; i < numModes; ++i) {
        t.p[i] = nranksPerMode ? nranksPerMode[i] : 1;
        if (extent[i] <= 0 || t.p[i] <= 0) return CUTENSOR_STATUS_INVALID_VALUE;
        t.bs[i] = blockSize ? blockSize[i] : (extent[i] + t.p[i] - 1) / t.p[i];
        if (t.bs[i] <= 0) return CUTENSOR_STATUS_INVALID_VALUE;
        if (t.bs[i] * t.p[i] < extent[i]) return CUTENSOR_STATUS_NOT_SUPPORTED;   // block-cyclic
        t.cellStride[i] = cells;
        cells *= t.p[i];
        t.elemStride[i] = elementStride ? elementStride[i] : run;
        if (t.elemStride[i] != run) t.packed = false;
        run *= t.bs[i];
    }
    t.numCells = cells;
    const int world = handle->transport->size();
    if (cells > 1) {
        if ((int64_t)nranks != cells || cells != world) return CUTENSOR_STATUS_INVALID_VALUE;
        t.owner.resize((size_t)cells);
        std::vector<char> seen((size_t)world, 0);
        for (int64_t c = 0; c < cells; ++c) {
            const int32_t r = ranks ? ranks[c] : (int32_t)c;
            if (r < 0 || r >= world || seen[(size_t)r]) return CUTENSOR_STATUS_INVALID_VALUE;   // one block per rank
            seen[(size_t)r] = 1;
            t.owner[(size_t)c] = r;
        }
    }
    *desc = d.release();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMpDestroyTensorDescriptor(cutensorMpTensorDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// cutensorMp_contraction.cu:485-488
cutensorStatus_t cutensorMpCreateContraction(const cutensorMpHandle_t handle, cutensorMpOperationDescriptor_t* desc,
                                             const cutensorMpTensorDescriptor_t descA, const int32_t modesA[], cutensorOperator_t opA,
                                             const cutensorMpTensorDescriptor_t descB, const int32_t modesB[], cutensorOperator_t opB,
                                             const cutensorMpTensorDescriptor_t descC, const int32_t modesC[], cutensorOperator_t opC,
                                             const cutensorMpTensorDescriptor_t descD, const int32_t modesD[],
                                             const cutensorComputeDescriptor_t compute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || descA == nullptr || descB == nullptr || descC == nullptr || descD == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if ((descA->t.n && !modesA) || (descB->t.n && !modesB) || (descC->t.n && (!modesC || !modesD))) return CUTENSOR_STATUS_INVALID_VALUE;
    std::unique_ptr<cutensorMpOperationDescriptor> d(new (std::nothrow) cutensorMpOperationDescriptor());
    if (d == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    d->A = descA->t; d->B = descB->t; d->C = descC->t;
    d->mA.assign(modesA, modesA + d->A.n);
    d->mB.assign(modesB, modesB + d->B.n);
    d->mC.assign(modesC, modesC + d->C.n);
    d->opA = opA; d->opB = opB; d->opC = opC;
    d->compute = compute;
    const MpTensor& D = descD->t;
    const std::vector<int32_t> mD(modesD, modesD + D.n);
    const bool sameCD = mD == d->mC && D.extent == d->C.extent && D.p == d->C.p && D.bs == d->C.bs &&
                        D.elemStride == d->C.elemStride && D.owner == d->C.owner && D.dtype == d->C.dtype;
    if (!sameCD || d->A.dtype != d->B.dtype || d->A.dtype != d->C.dtype) return CUTENSOR_STATUS_NOT_SUPPORTED;
    auto check = [&](const MpTensor& x, const std::vector<int32_t>& mx, const MpTensor& y, const std::vector<int32_t>& my) {
        for (uint32_t i = 0; i < x.n; ++i) {
            const int j = find_label(my, mx[i]);
            if (j >= 0 && x.extent[i] != y.extent[(size_t)j]) return false;
        }
        return true;
    };
    if (!check(d->A, d->mA, d->B, d->mB) || !check(d->A, d->mA, d->C, d->mC) || !check(d->B, d->mB, d->C, d->mC)) return CUTENSOR_STATUS_INVALID_VALUE;
    for (int32_t l : d->mC)
        if (find_label(d->mA, l) < 0 && find_label(d->mB, l) < 0) return CUTENSOR_STATUS_INVALID_VALUE;
    *desc = d.release();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMpDestroyOperationDescriptor(cutensorMpOperationDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// cutensorMp_contraction.cu:490-500
cutensorStatus_t cutensorMpCreatePlanPreference(const cutensorMpHandle_t handle, cutensorMpPlanPreference_t* pref,
                                                cutensorMpAlgo_t algo, uint64_t workspaceSizeDeviceLimit,
                                                uint64_t workspaceSizeHostLimit) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (pref == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (algo != CUTENSORMP_ALGO_DEFAULT) return CUTENSOR_STATUS_NOT_SUPPORTED;
    cutensorMpPlanPreference* p = new (std::nothrow) cutensorMpPlanPreference{algo, workspaceSizeDeviceLimit, workspaceSizeHostLimit};
    if (p == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    *pref = p;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMpDestroyPlanPreference(cutensorMpPlanPreference_t pref) try {
    delete pref;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// cutensorMp_contraction.cu:502-503
cutensorStatus_t cutensorMpCreatePlan(const cutensorMpHandle_t handle, cutensorMpPlan_t* plan,
                                      const cutensorMpOperationDescriptor_t desc, const cutensorMpPlanPreference_t pref) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || desc == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    DeviceGuard guard(handle->device);
    std::unique_ptr<cutensorMpPlan> pl(new (std::nothrow) cutensorMpPlan());
    if (pl == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    pl->desc = *desc;
    pl->rank = handle->transport->rank();
    pl->nranks = handle->transport->size();
    PlanContext c{handle, *pl, {}, pref ? pref->devLimit : (1ull << 62), {}};

    cutensorStatus_t st = own_c_boxes(c);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    if (choose_algorithm(c)) {
        pl->reduce.reset(new ReducePlan());
        pl->reduce->replicatedC = pl->desc.C.replicated();
        pl->reduce->cElems = whole_box(pl->desc.C.extent).volume();
        st = pl->reduce->replicatedC ? plan_reduce_replicated(c) : plan_reduce_scattered(c);
        if (st == CUTENSOR_STATUS_SUCCESS) st = plan_reduce_contraction(c);
    } else {
        pl->gather.reset(new GatherPlan());
        st = plan_transfers(c);
        if (st == CUTENSOR_STATUS_SUCCESS) st = plan_staging(c);
        if (st == CUTENSOR_STATUS_SUCCESS) st = plan_gather_contraction(c);
    }
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    *plan = pl.release();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// cutensorMp_contraction.cu:506-509
cutensorStatus_t cutensorMpPlanGetAttribute(const cutensorMpHandle_t handle, const cutensorMpPlan_t plan,
                                            cutensorMpPlanAttribute_t attr, void* buf, size_t sizeInBytes) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || buf == nullptr || sizeInBytes < sizeof(uint64_t)) return CUTENSOR_STATUS_INVALID_VALUE;
    switch (attr) {
        case CUTENSORMP_PLAN_REQUIRED_WORKSPACE_DEVICE: *static_cast<uint64_t*>(buf) = plan->requiredDevice; return CUTENSOR_STATUS_SUCCESS;
        case CUTENSORMP_PLAN_REQUIRED_WORKSPACE_HOST: *static_cast<uint64_t*>(buf) = 0; return CUTENSOR_STATUS_SUCCESS;
    }
    return CUTENSOR_STATUS_INVALID_VALUE;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMpDestroyPlan(cutensorMpPlan_t plan) try {
    delete plan;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// cutensorMp_contraction.cu:537-538
cutensorStatus_t cutensorMpContract(const cutensorMpHandle_t handle, const cutensorMpPlan_t plan, const void* alpha,
                                    const void* A, const void* B, const void* beta, const void* C, void* D,
                                    void* workspaceDevice, void* workspaceHost) try {
    (void)workspaceHost;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || alpha == nullptr || beta == nullptr || A == nullptr || B == nullptr || D == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (plan->requiredDevice > 0 && workspaceDevice == nullptr) return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
    if (handle->device < 0) return CUTENSOR_STATUS_ARCH_MISMATCH;   // plan-only handle of a machine without a GPU
    DeviceGuard guard(handle->device);
    const CallArgs a{alpha, A, B, beta, C, D, static_cast<char*>(workspaceDevice)};
    return plan->reduce ? run_reduce(handle, *plan, a) : run_gather(handle, *plan, a);
} CTAMD_API_CATCH

}  // extern "C"
