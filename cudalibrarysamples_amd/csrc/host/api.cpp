// api.cpp — the exported cuTENSOR C ABI (include/cutensor.h) of handles, descriptors and preferences on top of the planners: the handle
// with its plan-cache entry points (thin calls into PlanStore, plan_store.hpp), tensor and operation descriptors, the plan preference,
// the workspace estimate, the kernel-cache files, error strings and the version.  Plans are made in create_plan.cpp, contractions run
// in exec_contraction.cpp, the element-wise family in exec_elementwise.cpp, plans are described in describe.cpp.  Each entry point
// cites the reference call site it serves.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

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

}  // namespace

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
    if (handle != nullptr)
        for (auto& ev : handle->prof.events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (handle != nullptr && handle->syncPool != nullptr) (void)hipFree(handle->syncPool);
    delete handle;   // (the store destroys the event pairs of trials nobody read)
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// einsum.cu:445
cutensorStatus_t cutensorHandleResizePlanCache(cutensorHandle_t handle, const uint32_t numEntries) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    handle->plans.resize(numEntries);
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_plan_cache.cu:324-337 — one line per cached problem: key \t kernel \t splitK
cutensorStatus_t cutensorHandleWritePlanCacheToFile(const cutensorHandle_t handle, const char filename[]) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (filename == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    return handle->plans.write_file(filename);
} CTAMD_API_CATCH

// contraction_plan_cache.cu:132-148
cutensorStatus_t cutensorHandleReadPlanCacheFromFile(cutensorHandle_t handle, const char filename[],
                                                     uint32_t* numCachelinesRead) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (filename == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    return handle->plans.read_file(filename, numCachelinesRead);
} CTAMD_API_CATCH

// Plan-memo counters of this handle (not part of the cuTENSOR ABI): plans answered by cloning a prototype / plans that went through the
// planner / prototypes held.
void ctamdPlanMemoStats(const cutensorHandle_t handle, uint64_t* hits, uint64_t* misses, uint32_t* entries) try {
    if (handle == nullptr) return;
    const PlanStore::Stats s = handle->plans.stats();
    if (hits) *hits = s.hits;
    if (misses) *misses = s.misses;
    if (entries) *entries = s.entries;
} CTAMD_API_CATCH_VOID

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
    EwPlan ep;
    ReducePlan rp;
    std::string why;
    st = plan_elementwise_any(op, 0, handle->numCUs, ep, rp, &why);   // validates the problem
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
    ReducePlan rp;
    std::string why;
    st = plan_elementwise_any(op, 0, handle->numCUs, ep, rp, &why);
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
    ReducePlan rp;
    std::string why;
    st = plan_elementwise_any(op, 0, handle->numCUs, ep, rp, &why);
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
        EwPlan ep;
        ReducePlan rp;
        const cutensorStatus_t st = plan_elementwise_any(*desc, cap, handle->numCUs, ep, rp, nullptr);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        *workspaceSizeEstimate = rp.workspace;
    }
    return CUTENSOR_STATUS_SUCCESS;
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

}  // extern "C"
