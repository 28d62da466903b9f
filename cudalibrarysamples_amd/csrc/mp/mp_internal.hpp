// mp_internal.hpp — what the files of libcutensorMp.so share (overview: mp.cpp).
//   mp_geometry.h    boxes, offsets, copy modes and launches (integers only)
//   mp_transport.cpp the exchange layer: RCCL, and rank threads of one process on one GPU
//   mp_copy.cpp      strided copies through the single-GPU ABI
//   mp_plan.cpp      the plan builder's steps
//   mp_call.cpp      the two exchange algorithms of a call
//   mp_describe.cpp  ctamdMpDescribePlan
//   mp.cpp           handle, descriptors, preference; cutensorMpCreatePlan / cutensorMpContract as the sequence of their steps
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include <hip/hip_runtime.h>

#include <cutensor.h>
#include <cutensorMp.h>

#include "../host/api_guard.hpp"
#include "mp_geometry.h"

namespace ctamd_mp CTAMD_MP_HIDDEN {

inline size_t elem_size(hipDataType t) {
    switch (t) {
        case HIP_R_16F: case HIP_R_16BF: return 2;
        case HIP_R_32F: return 4;
        case HIP_R_64F: case HIP_C_32F: return 8;
        case HIP_C_64F: return 16;
        default: return 0;
    }
}
inline bool is_complex(hipDataType t) { return t == HIP_C_32F || t == HIP_C_64F; }
inline hipDataType real_type(hipDataType t) { return t == HIP_C_32F ? HIP_R_32F : t == HIP_C_64F ? HIP_R_64F : t; }
// The type of alpha / beta, which is not always the data type: fp32 data with CUTENSOR_COMPUTE_DESC_64F takes double scalars, complex
// data complex ones — the single-GPU layer's rule (host/api.cpp, scalar_type_for).
inline hipDataType scalar_type(hipDataType data, cutensorComputeDescriptor_t compute) {
    if (is_complex(data)) return data;
    return (data == HIP_R_64F || compute == CUTENSOR_COMPUTE_DESC_64F) ? HIP_R_64F : HIP_R_32F;
}
// the scalar 1 of an element-wise operation on data of real type `realType` (double for fp64, float for everything narrower)
inline const void* one_of(hipDataType realType) {
    static const float onef = 1.f;
    static const double oned = 1.0;
    return realType == HIP_R_64F ? static_cast<const void*>(&oned) : static_cast<const void*>(&onef);
}

class DeviceGuard {   // the caller's current device is restored; `device` >= 0 is made current meanwhile
public:
    explicit DeviceGuard(int device = -1) {
        (void)hipGetDevice(&saved_);
        if (device >= 0) (void)hipSetDevice(device);
    }
    ~DeviceGuard() { if (saved_ >= 0) (void)hipSetDevice(saved_); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
private:
    int saved_ = -1;
};

// ---- ownership of single-GPU objects -------------------------------------------------------------------------------
struct EnginePlanDeleter { void operator()(cutensorPlan_t p) const { cutensorDestroyPlan(p); } };
using EnginePlan = std::unique_ptr<cutensorPlan, EnginePlanDeleter>;
// the descriptors, operation and preference a planning step makes on the way to a single-GPU plan: released when the step ends
struct EngineTemps {
    cutensorTensorDescriptor_t desc[3] = {nullptr, nullptr, nullptr};
    cutensorOperationDescriptor_t op = nullptr;
    cutensorPlanPreference_t pref = nullptr;
    EngineTemps() = default;
    EngineTemps(const EngineTemps&) = delete;
    EngineTemps& operator=(const EngineTemps&) = delete;
    ~EngineTemps() {
        cutensorDestroyPlanPreference(pref);
        cutensorDestroyOperationDescriptor(op);
        for (auto d : desc) cutensorDestroyTensorDescriptor(d);
    }
};

// ---- exchange layer (mp_transport.cpp) -----------------------------------------------------------------------------
class Transport {
public:
    virtual ~Transport() {}
    virtual int rank() const = 0;
    virtual int size() const = 0;
    virtual bool begin() = 0;
    virtual bool send(const void* buf, size_t bytes, int peer, hipStream_t s) = 0;
    virtual bool recv(void* buf, size_t bytes, int peer, hipStream_t s) = 0;
    virtual bool end(hipStream_t s) = 0;
    // sums of `count` elements of the real type `t`; scratch: `count` elements, used by transports that need it
    virtual bool all_reduce(void* buf, size_t count, hipDataType t, void* scratch, hipStream_t s) = 0;
    virtual bool reduce_scatter(const void* send, void* recv, size_t countPerRank, hipDataType t, hipStream_t s) = 0;
    virtual bool needs_scratch() const { return false; }
    virtual void set_engine(cutensorHandle_t) {}     // the single-GPU handle a transport may run its own element-wise sums on
};
struct LocalWorld;                                    // several ranks as threads of one process on one GPU
LocalWorld* new_local_world(int nranks);              // nullptr: out of memory
void delete_local_world(LocalWorld* w);
int local_world_size(const LocalWorld* w);
bool rccl_rank_and_size(ncclComm_t comm, int* rank, int* size);    // false: not a usable communicator
Transport* new_rccl_transport(ncclComm_t comm, int rank, int size);
Transport* new_local_transport(LocalWorld* w, int rank);

// ---- strided copies through the single-GPU ABI (mp_copy.cpp) ----------------------------------------------------------
struct CopyOp {                // move-only: owns its plan
    EnginePlan plan;
    Launches launches;
};
// Builds the copy of a box that starts srcBase / dstBase elements into its buffers; when the element-wise planner rejects the view
// (too many unfusable modes) the smallest mode is peeled into a host loop over launches of the remaining view.
cutensorStatus_t make_copy(cutensorHandle_t h, hipDataType dtype, const std::vector<CMode>& modes, CopyOp& op, int64_t srcBase = 0, int64_t dstBase = 0);
cutensorStatus_t run_copy(cutensorHandle_t h, const CopyOp& c, hipDataType dtype, const void* src, void* dst, hipStream_t s);

// ---- plan ------------------------------------------------------------------------------------------------------------
struct Region { int64_t off = 0, bytes = 0; };       // of the device workspace; off is a multiple of 256
class WorkspaceLayout {                               // hands out regions in order, each rounded up to 256 bytes
public:
    Region take(int64_t bytes) { Region r{end_, bytes}; end_ += round_up(bytes, 256); return r; }
    int64_t end() const { return end_; }
private:
    int64_t end_ = 0;
};

struct Transfer {            // one sub-box of operand `tensor` (0 = A, 1 = B) moving from rank `src` to rank `dst`
    int tensor, src, dst;
    Box box;
    int64_t bytes;
    // sender side
    bool direct = false;     // sent straight from the user's block (whole, contiguous)
    int64_t sendOff = 0;     // byte offset in the workspace (packed transfers)
    CopyOp pack;
    // receiver side
    bool inPlace = false;    // received straight into the staging tensor (single source covering the whole box)
    int64_t recvOff = 0;     // byte offset in the workspace: in the receive region, or the operand's staging tensor when inPlace
    CopyOp unpack;
};

struct OperandPlan {
    bool staged = false;             // false: the local contraction reads the user's block in place
    Box need;
    int64_t viewOff = 0;             // element offset of the view inside the user's block (in-place only)
    std::vector<int64_t> viewStride;
    Region stage;                    // the dense staging tensor (staged only)
    std::vector<CopyOp> localCopies; // own block -> staging
};

// "owner computes, gather what you need" (see mp.cpp).  Workspace: send | recv | stage | contraction workspace.
struct GatherPlan {
    std::vector<Transfer> sends, recvs;     // in issue order (tensor-major, then peer / cell) — identical on both sides
    OperandPlan in[2];
    Region send, recv, stage;
};

// "stationary inputs, reduce the result" (see mp.cpp).  Workspace: stage, scratch (replicated C) or stage, send, recv (distributed C),
// then the contraction workspace.
struct ReducePlan {
    bool replicatedC = false;
    bool direct = false;             // replicated C, packed: contract and all-reduce in the user's D
    int64_t cElems = 0;              // elements of the whole C
    Region stage;                    // the full-size partial of C
    CopyOp cIn;                      // beta != 0: the rank's (block of) C -> partial
    CopyOp out;                      // replicated, not direct: reduced partial -> D
    bool packDirect = false;         // the destination blocks are already equal contiguous slots of the partial
    std::vector<CopyOp> pack;        // partial -> slot q of the send region
    Region send;
    int64_t slotElems = 0;
    bool recvDirect = false;         // the rank's D block is a packed slot: reduce-scatter straight into it
    Region recv;
    CopyOp unpack;                   // received slot -> D block
    Region scratch;
};

struct TensorView { std::vector<int64_t> extent, stride; uint32_t align; };   // an operand of the local contraction

}  // namespace ctamd_mp

struct cutensorMpHandle {
    std::unique_ptr<ctamd_mp::Transport> transport;
    int device = 0;
    hipStream_t stream = nullptr;
    cutensorHandle_t h = nullptr;
    ~cutensorMpHandle() { if (h) cutensorDestroy(h); }
};
struct cutensorMpTensorDescriptor { ctamd_mp::MpTensor t; };
struct cutensorMpOperationDescriptor {
    ctamd_mp::MpTensor A, B, C;
    std::vector<int32_t> mA, mB, mC;
    cutensorOperator_t opA, opB, opC;
    cutensorComputeDescriptor_t compute;
    const ctamd_mp::MpTensor& operand(int k) const { return k == 0 ? A : k == 1 ? B : C; }
    const std::vector<int32_t>& modes(int k) const { return k == 0 ? mA : k == 1 ? mB : mC; }
};
struct cutensorMpPlanPreference { cutensorMpAlgo_t algo; uint64_t devLimit, hostLimit; };
struct cutensorMpPlan {
    cutensorMpOperationDescriptor desc;
    int rank = 0, nranks = 1;
    bool compute = false;                       // this rank runs the local contraction
    int64_t gatherTotal = 0, reduceTotal = 0;   // bytes on the wire over all ranks, per algorithm (the selection rule)
    std::unique_ptr<ctamd_mp::GatherPlan> gather;   // exactly one of the two: the algorithm
    std::unique_ptr<ctamd_mp::ReducePlan> reduce;
    ctamd_mp::EnginePlan contraction;
    uint64_t contractionWs = 0;
    int64_t contractionOff = 0;                 // byte offset of the contraction's workspace: behind the algorithm's regions
    uint64_t requiredDevice = 0;
};

namespace ctamd_mp CTAMD_MP_HIDDEN {

// ---- the plan builder's steps (mp_plan.cpp), in the order cutensorMpCreatePlan takes them ---------------------------------
struct PlanContext {                         // what every step reads
    cutensorMpHandle* handle;
    cutensorMpPlan& pl;
    std::vector<Box> cBox;                   // the box of C every rank owns
    uint64_t devLimit;
    WorkspaceLayout ws;
};
cutensorStatus_t own_c_boxes(PlanContext& c);
bool choose_algorithm(PlanContext& c);       // true: reduce.  Fills gatherTotal / reduceTotal.
cutensorStatus_t plan_transfers(PlanContext& c);
cutensorStatus_t plan_staging(PlanContext& c);
cutensorStatus_t plan_gather_contraction(PlanContext& c);
cutensorStatus_t plan_reduce_replicated(PlanContext& c);
cutensorStatus_t plan_reduce_scattered(PlanContext& c);
cutensorStatus_t plan_reduce_contraction(PlanContext& c);
// The local contraction over three views, its workspace capped by `budget`; fills contraction, contractionWs, contractionOff and
// requiredDevice.
cutensorStatus_t plan_local_contraction(PlanContext& c, const TensorView (&view)[3], uint64_t budget);

// ---- a call (mp_call.cpp) ---------------------------------------------------------------------------------------------
struct CallArgs { const void* alpha; const void* A; const void* B; const void* beta; const void* C; void* D; char* ws; };
cutensorStatus_t run_gather(cutensorMpHandle* handle, const cutensorMpPlan& plan, const CallArgs& a);
cutensorStatus_t run_reduce(cutensorMpHandle* handle, const cutensorMpPlan& plan, const CallArgs& a);

}  // namespace ctamd_mp
