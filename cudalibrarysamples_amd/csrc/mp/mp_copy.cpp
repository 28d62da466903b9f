// mp_copy.cpp — strided copies of boxes through the single-GPU ABI: an identity cutensorPermute per launch.
#include <cstring>

#include "mp_internal.hpp"

extern "C" int ctamdDescribePlan(const cutensorPlan_t plan, char* buf, size_t len);   // libcutensor.so diagnostic

namespace ctamd_mp CTAMD_MP_HIDDEN {

// A copy of more unfusable modes than the tiled element-wise kernels describe used to be refused, and make_copy peels modes until one
// is not; the single-GPU library now plans such a copy on its mode-table kernels instead.  The launch counts of this library's plans
// are pinned, so a plan on those kernels is still the refusal it used to be — exactly so: that route starts only where the refusal was.
static bool on_mode_table(cutensorPlan_t plan) {
    char text[1024];
    return ctamdDescribePlan(plan, text, sizeof(text)) > 0 && std::strstr(text, "\"kname\":\"ew_table_") != nullptr;
}

static cutensorStatus_t try_copy_plan(cutensorHandle_t h, hipDataType dtype, const std::vector<CMode>& modes, uint32_t alignSrc, uint32_t alignDst,
                                      EnginePlan& plan) {
    // complex data is copied as pairs of reals: a leading stride-1 mode of extent 2
    const hipDataType rt = real_type(dtype);
    const int64_t scale = is_complex(dtype) ? 2 : 1;
    std::vector<int64_t> ext, sS, sD;
    std::vector<int32_t> lab;
    if (scale == 2) { ext.push_back(2); sS.push_back(1); sD.push_back(1); lab.push_back(0); }
    for (const CMode& m : modes) { ext.push_back(m.extent); sS.push_back(m.sSrc * scale); sD.push_back(m.sDst * scale); lab.push_back((int32_t)lab.size() + 1); }
    EngineTemps tmp;
    cutensorPlan_t raw = nullptr;
    cutensorStatus_t st = cutensorCreateTensorDescriptor(h, &tmp.desc[0], (uint32_t)ext.size(), ext.data(), sS.data(), rt, alignSrc);
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreateTensorDescriptor(h, &tmp.desc[1], (uint32_t)ext.size(), ext.data(), sD.data(), rt, alignDst);
    if (st == CUTENSOR_STATUS_SUCCESS)
        st = cutensorCreatePermutation(h, &tmp.op, tmp.desc[0], lab.data(), CUTENSOR_OP_IDENTITY, tmp.desc[1], lab.data(),
                                       rt == HIP_R_64F ? CUTENSOR_COMPUTE_DESC_64F : CUTENSOR_COMPUTE_DESC_32F);
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlan(h, &raw, tmp.op, nullptr, 0);
    if (st == CUTENSOR_STATUS_SUCCESS && on_mode_table(raw)) {
        cutensorDestroyPlan(raw);
        raw = nullptr;
        st = CUTENSOR_STATUS_NOT_SUPPORTED;
    }
    plan.reset(raw);
    return st;
}

cutensorStatus_t make_copy(cutensorHandle_t h, hipDataType dtype, const std::vector<CMode>& modes, CopyOp& op, int64_t srcBase, int64_t dstBase) {
    std::vector<CMode> g = fuse_modes(modes);
    const int64_t es = (int64_t)elem_size(dtype);
    op.launches.assign(1, std::make_pair(srcBase, dstBase));
    for (;;) {
        cutensorStatus_t st = try_copy_plan(h, dtype, g, common_alignment(op.launches, false, es), common_alignment(op.launches, true, es), op.plan);
        if (st == CUTENSOR_STATUS_SUCCESS) return st;
        if (st != CUTENSOR_STATUS_NOT_SUPPORTED || g.empty()) return st;
        if (!peel_smallest_mode(g, op.launches)) return CUTENSOR_STATUS_NOT_SUPPORTED;
    }
}

cutensorStatus_t run_copy(cutensorHandle_t h, const CopyOp& c, hipDataType dtype, const void* src, void* dst, hipStream_t s) {
    const void* one = one_of(real_type(dtype));
    const int64_t es = (int64_t)elem_size(dtype);
    for (const auto& l : c.launches) {
        cutensorStatus_t st = cutensorPermute(h, c.plan.get(), one, static_cast<const char*>(src) + l.first * es,
                                              static_cast<char*>(dst) + l.second * es, s);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
    }
    return CUTENSOR_STATUS_SUCCESS;
}

}  // namespace ctamd_mp
