// einsum_c.cpp — C entry points over cutensor_amd::Einsum<> so that Python (ctypes) can drive the
// same C++ helper the native samples use.  The reference exposes its helper to Python through
// pybind11 (cuTENSOR/python/cutensor/torch/einsum.cc:75-137); this is the same seam without a
// framework dependency: plain pointers and sizes only.
#include <cstring>
#include <new>

#include "einsum.hpp"
#include "../host/api_guard.hpp"

namespace {
constexpr int kMaxModes = 64;   // torch/einsum.cc:84
struct Base {
    virtual ~Base() {}
    virtual bool init() const = 0;
    virtual std::vector<int64_t> shape() const = 0;
    virtual bool plan(cutensorHandle_t h, uint64_t limit) = 0;
    virtual bool replan(cutensorHandle_t h, uint64_t limit) = 0;
    virtual uint64_t required() const = 0;
    virtual bool exec(cutensorHandle_t h, const void* A, const void* B, void* C, void* w, hipStream_t s) = 0;
    virtual cutensorPlan_t raw() const = 0;
    virtual void conj(bool a, bool b) = 0;
    virtual void compute(cutensorComputeDescriptor_t c) = 0;
};
template <typename T>
struct Impl : Base {
    cutensor_amd::Einsum<T, int64_t, kMaxModes> e;
    Impl(const char* eq, const std::vector<int64_t>& a, const std::vector<int64_t>& b) : e(eq, a, b) {}
    bool init() const override { return e.isInitialized(); }
    std::vector<int64_t> shape() const override { return e.getOutputShape(); }
    bool plan(cutensorHandle_t h, uint64_t limit) override { return e.plan(h, limit); }
    bool replan(cutensorHandle_t h, uint64_t limit) override { return e.replan(h, limit); }
    uint64_t required() const override { return e.requiredWorkspace(); }
    bool exec(cutensorHandle_t h, const void* A, const void* B, void* C, void* w, hipStream_t s) override {
        return e.execute(h, A, B, C, w, s);
    }
    cutensorPlan_t raw() const override { return e.rawPlan(); }
    void conj(bool a, bool b) override { e.setConjugate(a, b); }
    void compute(cutensorComputeDescriptor_t c) override { e.setComputeDescriptor(c); }
};
// One real fp64 operand, the other one and the output complex128 (the mixed rows of the contraction type table): the equation is parsed by
// Einsum<std::complex<double>>, which is never planned itself; descriptors, plan and execution are this struct's, with one data type per
// operand, complex double scalars and COMPUTE_DESC_64F.
struct MixedImpl : Base {
    cutensor_amd::Einsum<std::complex<double>, int64_t, kMaxModes> e;
    std::vector<int64_t> extA, extB;      // cuTENSOR order (reversed)
    cutensorDataType_t typeA, typeB;
    bool conjA = false, conjB = false, refused = false;
    cutensorPlan_t plan_ = nullptr;
    uint64_t required_ = 0;
    MixedImpl(const char* eq, const std::vector<int64_t>& a, const std::vector<int64_t>& b, cutensorDataType_t ta, cutensorDataType_t tb)
        : e(eq, a, b), extA(a.rbegin(), a.rend()), extB(b.rbegin(), b.rend()), typeA(ta), typeB(tb) {}
    ~MixedImpl() override { if (plan_) cutensorDestroyPlan(plan_); }
    bool init() const override { return e.isInitialized() && !e.modesB().empty(); }
    std::vector<int64_t> shape() const override { return e.getOutputShape(); }
    bool plan(cutensorHandle_t h, uint64_t limit) override {
        if (!init() || refused) return false;
        if (plan_) return true;
        const uint32_t kAlignment = 128;
        cutensorTensorDescriptor_t dA = nullptr, dB = nullptr, dC = nullptr;
        cutensorOperationDescriptor_t op = nullptr;
        cutensorPlanPreference_t pref = nullptr;
        bool ok = cutensorCreateTensorDescriptor(h, &dA, (uint32_t)extA.size(), extA.data(), nullptr, typeA, kAlignment) == CUTENSOR_STATUS_SUCCESS &&
                  cutensorCreateTensorDescriptor(h, &dB, (uint32_t)extB.size(), extB.data(), nullptr, typeB, kAlignment) == CUTENSOR_STATUS_SUCCESS &&
                  cutensorCreateTensorDescriptor(h, &dC, (uint32_t)e.extentC().size(), e.extentC().data(), nullptr, CUTENSOR_C_64F, kAlignment) == CUTENSOR_STATUS_SUCCESS &&
                  cutensorCreatePlanPreference(h, &pref, CUTENSOR_ALGO_DEFAULT, CUTENSOR_JIT_MODE_NONE) == CUTENSOR_STATUS_SUCCESS &&
                  cutensorCreateContraction(h, &op, dA, e.modesA().data(), conjA ? CUTENSOR_OP_CONJ : CUTENSOR_OP_IDENTITY, dB, e.modesB().data(),
                                            conjB ? CUTENSOR_OP_CONJ : CUTENSOR_OP_IDENTITY, dC, e.modesC().data(), CUTENSOR_OP_IDENTITY, dC,
                                            e.modesC().data(), CUTENSOR_COMPUTE_DESC_64F) == CUTENSOR_STATUS_SUCCESS &&
                  cutensorCreatePlan(h, &plan_, op, pref, limit) == CUTENSOR_STATUS_SUCCESS &&
                  cutensorPlanGetAttribute(h, plan_, CUTENSOR_PLAN_REQUIRED_WORKSPACE, &required_, sizeof(required_)) == CUTENSOR_STATUS_SUCCESS;
        cutensorDestroyOperationDescriptor(op);
        cutensorDestroyPlanPreference(pref);
        cutensorDestroyTensorDescriptor(dA);
        cutensorDestroyTensorDescriptor(dB);
        cutensorDestroyTensorDescriptor(dC);
        if (!ok && plan_) { cutensorDestroyPlan(plan_); plan_ = nullptr; }
        return ok;
    }
    bool replan(cutensorHandle_t h, uint64_t limit) override {
        if (plan_) { cutensorDestroyPlan(plan_); plan_ = nullptr; }
        required_ = 0;
        return plan(h, limit);
    }
    uint64_t required() const override { return required_; }
    bool exec(cutensorHandle_t h, const void* A, const void* B, void* C, void* w, hipStream_t s) override {
        if (!plan_) return false;
        const std::complex<double> alpha = 1, beta = 0;
        return cutensorContract(h, plan_, &alpha, A, B, &beta, C, C, w, required_, s) == CUTENSOR_STATUS_SUCCESS;
    }
    cutensorPlan_t raw() const override { return plan_; }
    void conj(bool a, bool b) override { conjA = a; conjB = b; }
    void compute(cutensorComputeDescriptor_t c) override { refused = c != nullptr && c != CUTENSOR_COMPUTE_DESC_64F; }      // 64F only
};
}  // namespace

extern "C" {

void* ctamdEinsumCreate(const char* equation, const int64_t* shapeA, int nA, const int64_t* shapeB, int nB, int dtype) try {
    if (equation == nullptr || nA < 0 || nB < 0) return nullptr;
    std::vector<int64_t> a(shapeA, shapeA + nA), b(shapeB, shapeB + nB);
    switch (dtype) {
        case HIP_R_32F:  return static_cast<Base*>(new (std::nothrow) Impl<float>(equation, a, b));
        case HIP_R_64F:  return static_cast<Base*>(new (std::nothrow) Impl<double>(equation, a, b));
        case HIP_R_16F:  return static_cast<Base*>(new (std::nothrow) Impl<__half>(equation, a, b));
        case HIP_R_16BF: return static_cast<Base*>(new (std::nothrow) Impl<__hip_bfloat16>(equation, a, b));
        case HIP_C_32F:  return static_cast<Base*>(new (std::nothrow) Impl<std::complex<float>>(equation, a, b));
        case HIP_C_64F:  return static_cast<Base*>(new (std::nothrow) Impl<std::complex<double>>(equation, a, b));
        default: return nullptr;
    }
} CTAMD_API_CATCH_NULL
// one data type per operand: equal types as ctamdEinsumCreate; else one of (R_64F, C_64F) / (C_64F, R_64F) — a two-operand contraction into
// a complex128 output.  Any other pair: null.
void* ctamdEinsumCreateTyped(const char* equation, const int64_t* shapeA, int nA, const int64_t* shapeB, int nB, int dtypeA, int dtypeB) try {
    if (dtypeA == dtypeB) return ctamdEinsumCreate(equation, shapeA, nA, shapeB, nB, dtypeA);
    if (equation == nullptr || nA < 0 || nB < 0) return nullptr;
    if (!((dtypeA == HIP_R_64F && dtypeB == HIP_C_64F) || (dtypeA == HIP_C_64F && dtypeB == HIP_R_64F))) return nullptr;
    std::vector<int64_t> a(shapeA, shapeA + nA), b(shapeB, shapeB + nB);
    return static_cast<Base*>(new (std::nothrow) MixedImpl(equation, a, b, (cutensorDataType_t)dtypeA, (cutensorDataType_t)dtypeB));
} CTAMD_API_CATCH_NULL
void ctamdEinsumDestroy(void* e) try { delete static_cast<Base*>(e); } CTAMD_API_CATCH_VOID
void ctamdEinsumSetConjugate(void* e, int conjA, int conjB) try { if (e) static_cast<Base*>(e)->conj(conjA != 0, conjB != 0); } CTAMD_API_CATCH_VOID
// compute descriptor by its index (0 16F, 1 16BF, 2 TF32, 3 3XTF32, 4 32F, 5 64F; anything else: the data type's default); before ctamdEinsumPlan
void ctamdEinsumSetCompute(void* e, int id) try {
    static const cutensorComputeDescriptor_t* const kDesc[6] = {&CUTENSOR_COMPUTE_DESC_16F, &CUTENSOR_COMPUTE_DESC_16BF, &CUTENSOR_COMPUTE_DESC_TF32,
                                                                &CUTENSOR_COMPUTE_DESC_3XTF32, &CUTENSOR_COMPUTE_DESC_32F, &CUTENSOR_COMPUTE_DESC_64F};
    if (e) static_cast<Base*>(e)->compute((id >= 0 && id < 6) ? *kDesc[id] : nullptr);
} CTAMD_API_CATCH_VOID
int ctamdEinsumIsInitialized(void* e) try { return e && static_cast<Base*>(e)->init() ? 1 : 0; } CTAMD_API_CATCH_INT
int ctamdEinsumOutputShape(void* e, int64_t* out, int cap) try {
    if (!e) return -1;
    const std::vector<int64_t> s = static_cast<Base*>(e)->shape();
    for (size_t i = 0; i < s.size() && (int)i < cap; ++i) out[i] = s[i];
    return (int)s.size();
} CTAMD_API_CATCH_INT
int ctamdEinsumPlan(void* e, cutensorHandle_t h, uint64_t limit, uint64_t* required) try {
    if (!e || !static_cast<Base*>(e)->plan(h, limit)) return 0;
    if (required) *required = static_cast<Base*>(e)->required();
    return 1;
} CTAMD_API_CATCH_INT
// einsum.cc:104-123: plan again under a smaller workspace limit (0 = CUTENSOR_WORKSPACE_MIN) after an allocation failure
int ctamdEinsumReplan(void* e, cutensorHandle_t h, uint64_t limit, uint64_t* required) try {
    if (!e || !static_cast<Base*>(e)->replan(h, limit)) return 0;
    if (required) *required = static_cast<Base*>(e)->required();
    return 1;
} CTAMD_API_CATCH_INT
int ctamdEinsumExecute(void* e, cutensorHandle_t h, const void* A, const void* B, void* C, void* work, hipStream_t stream) try {
    return (e && static_cast<Base*>(e)->exec(h, A, B, C, work, stream)) ? 1 : 0;
} CTAMD_API_CATCH_INT
cutensorPlan_t ctamdEinsumRawPlan(void* e) try { return e ? static_cast<Base*>(e)->raw() : nullptr; } CTAMD_API_CATCH_NULL

}  // extern "C"
