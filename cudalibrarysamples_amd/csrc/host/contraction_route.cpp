// contraction_route.cpp — how a contraction runs: reduce lone modes first, peel, mode-table kernel, ranked tiled candidates, repack,
// a tiled family or the simple kernel.  The plan builders (create_plan.cpp) and cutensorEstimateWorkspaceSize take their decisions from here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "internal.hpp"

namespace ctamd {

// the kernel table a ContractionChoice::kernel of `family` indexes
const GettKernelInfo* kernel_table(int family, int* count) { return family == 2 ? gett_gen_kernels(count) : family == 1 ? gett_h16_kernels(count) : gett_f32_kernels(count); }
// ... and the entry itself; nullptr when `kernel` is not an index into that table
const GettKernelInfo* kernel_info(int family, int kernel) {
    int n = 0;
    const GettKernelInfo* tab = kernel_table(family, &n);
    return (kernel >= 0 && kernel < n) ? &tab[kernel] : nullptr;
}

// Peeling of a "wide" contraction (a group with more than kMaxGroupModes unfusable modes would run on the functional
// mode-table kernel, measured ~100x slower than the tiled ones): labels of the oversized groups are taken out of the problem,
// smallest extent first, until the rest fits the tiled kernels — at most kMaxPeelLaunches index combinations, each one launch of
// the same inner plan on offset operands.  Returns false when the problem is not wide for that reason or would take more launches.
static constexpr int64_t kMaxPeelLaunches = 64;
static bool peel_wide_contraction(const cutensorOperationDescriptor& desc, cutensorOperationDescriptor& inner, std::vector<PeelMode>& peel) {
    if (desc.kind != OpKind::Contraction) return false;
    inner = desc;
    peel.clear();
    // 16-bit data: a peeled CONTRACTED mode would accumulate through D, i.e. round every partial sum to the 16-bit type — the
    // kernels' contract is fp32 accumulation and ONE rounding.  Only free / batch modes are peeled for these types; an oversized K
    // group stays with the mode-table kernel (which accumulates in full precision).
    const bool h16 = dtype_size(desc.A.desc.dtype) == 2;
    int64_t launches = 1;
    auto idx = [](const TensorUse& t, int32_t l) { for (size_t i = 0; i < t.modes.size(); ++i) if (t.modes[i] == l) return (int)i; return -1; };
    for (int round = 0; round < 16; ++round) {
        ContractionView v;
        if (build_contraction_view(inner, v, nullptr) != CUTENSOR_STATUS_SUCCESS) return false;
        if (!v.wide) return !peel.empty();
        const std::vector<CanonMode>* gs[4] = {&v.L, &v.M, &v.N, &v.K};
        int32_t bestLabel = 0;
        int64_t bestExtent = 0;
        for (int g = 0; g < 4; ++g) {
            if ((int)gs[g]->size() <= kMaxGroupModes) continue;
            if (g == 3 && h16) return false;
            for (const CanonMode& m : *gs[g]) {
                // the label's own extent (a canonical mode may be a fused run; peeling its first label shortens the run)
                const int ia = idx(inner.A, m.label), ib = idx(inner.B, m.label), ic = idx(inner.C, m.label);
                const int64_t e = ia >= 0 ? inner.A.desc.extent[(size_t)ia] : ib >= 0 ? inner.B.desc.extent[(size_t)ib] : ic >= 0 ? inner.C.desc.extent[(size_t)ic] : 0;
                if (e < 2) continue;
                if (bestExtent == 0 || e < bestExtent) { bestLabel = m.label; bestExtent = e; }
            }
        }
        if (bestExtent == 0) return false;                       // wide for another reason (>= 2^31 elements in a group)
        launches *= bestExtent;
        if (launches > kMaxPeelLaunches) return false;
        const int32_t l = bestLabel;
        PeelMode pm;
        pm.extent = bestExtent;
        const int ia = idx(inner.A, l), ib = idx(inner.B, l), ic = idx(inner.C, l), id = idx(inner.D, l);
        if (ia >= 0) { pm.sA = inner.A.desc.stride[(size_t)ia]; inner.A.desc.extent[(size_t)ia] = 1; }
        if (ib >= 0) { pm.sB = inner.B.desc.stride[(size_t)ib]; inner.B.desc.extent[(size_t)ib] = 1; }
        if (ic >= 0) { pm.sC = inner.C.desc.stride[(size_t)ic]; inner.C.desc.extent[(size_t)ic] = 1; }
        if (id >= 0) { pm.sD = inner.D.desc.stride[(size_t)id]; inner.D.desc.extent[(size_t)id] = 1; }
        pm.contracted = (ic < 0);
        peel.push_back(pm);
    }
    return false;
}
// Contractions with a mode that ONE input carries and nothing else ('ijk,kl->il': j).  cutensorCreateContraction's GEMM view has no
// group for such a mode, but the reference's N-ary front end builds exactly these steps — _compute_target_tensor drops every mode no
// later operand or the target needs (cuTENSOR/python/cutensor/torch/einsum.py:111-156) — and torch.einsum, its comparator, sums the
// mode away.  Here: the operand is reduced over its lone modes first (cutensorReduce, OP_ADD) into a packed temporary in the workspace,
// then the ordinary contraction runs on the temporary.  (Summing first is also the cheap order: the contraction shrinks by the mode's
// extent.)  Returns false when the descriptor has no such mode; fills `inner` (the contraction on the temporaries) and the
// reductions otherwise.
// the packed temporary an operand X is reduced or copied into: a piece of the workspace at a multiple of 256 bytes, as aligned as the
// workspace itself (contraction.cu:242 asserts 128); its modes are pushed fastest first
struct PackedTemporary {
    TensorUse use;
    int64_t   elems = 1;
    explicit PackedTemporary(const TensorUse& X) { use.present = true; use.op = X.op; use.desc.dtype = X.desc.dtype; use.desc.alignment = 128; }
    void push(int32_t label, int64_t extent) {
        use.modes.push_back(label); use.desc.extent.push_back(extent); use.desc.stride.push_back(elems);
        use.desc.numModes += 1; elems *= extent;
    }
    uint64_t bytes() const { return (uint64_t)elems * dtype_size(use.desc.dtype); }
};
bool split_lone_modes(const cutensorOperationDescriptor& desc, TwoStepSplit& out) {
    auto has = [](const std::vector<int32_t>& v, int32_t l) { return std::find(v.begin(), v.end(), l) != v.end(); };
    auto reduce_operand = [&](const TensorUse& X, const TensorUse& other, cutensorOperationDescriptor& red, TensorUse& kept, uint64_t& bytes,
                              int64_t& summed) {
        bool lone = false;
        for (size_t i = 0; i < X.modes.size(); ++i)
            if (X.desc.extent[i] != 1 && !has(other.modes, X.modes[i]) && !has(desc.C.modes, X.modes[i])) lone = true;
        if (!lone) return false;
        PackedTemporary t(X);                                   // (it keeps X's operator: conj(sum) = sum(conj), the inner contraction conjugates)
        summed = 1;
        for (size_t i = 0; i < X.modes.size(); ++i) {
            if (!has(other.modes, X.modes[i]) && !has(desc.C.modes, X.modes[i])) summed *= X.desc.extent[i];   // summed away (extent-1 lone modes too)
            else t.push(X.modes[i], X.desc.extent[i]);
        }
        kept = t.use;
        bytes = t.bytes();
        red = cutensorOperationDescriptor{};
        red.kind = OpKind::Reduction;
        red.A = X;
        red.A.op = CUTENSOR_OP_IDENTITY;
        red.C = kept; red.C.op = CUTENSOR_OP_IDENTITY;
        red.D = red.C;
        red.opReduce = CUTENSOR_OP_ADD;
        red.compute = desc.compute;
        // (the real input of a mixed fp64 x complex128 contraction is summed as what it is: a real fp64 reduction, double scalars)
        red.scalarType = (X.desc.dtype == HIP_R_64F && desc.scalarType == HIP_C_64F) ? HIP_R_64F : desc.scalarType;
        return true;
    };
    TensorUse keptA, keptB;
    out.hasA = reduce_operand(desc.A, desc.B, out.stepA, keptA, out.bytesA, out.summedA);
    out.hasB = reduce_operand(desc.B, desc.A, out.stepB, keptB, out.bytesB, out.summedB);
    if (!out.hasA && !out.hasB) return false;
    out.inner = desc;
    if (out.hasA) out.inner.A = keptA;
    if (out.hasB) out.inner.B = keptB;
    return true;
}

// Repacked operands (round 6).  A 16-bit contraction whose operands the LDS-DMA kernels cannot stage in 16-byte units — an operand that is
// contiguous in a mode the K order does not start with ('ijk,lkj->il': A contiguous in k, B in j; the reference's 'mlik,lkjm->lij'), or in
// no staged mode at all — runs on the general family at 2-byte gathers: 70 TFLOP/s at 4096^2 x 1152 where the vendor BLAS reaches 630.
// When the problem is large enough to pay for it, the operand is copied FIRST (cutensorPermute, ~5 TB/s) into a packed temporary in the
// workspace — contracted modes fastest, in the order of the other operand's strides, then its free modes in D's order, then the batch
// modes — and the contraction runs on the temporaries on the LDS-DMA kernels.  (The reference library's own heuristics are closed; its
// samples only require that any stride pattern is accepted: cuTENSOR/contraction.cu:33-59.)  Decided by a time model: the copies at
// 4 TB/s + 4 us each + the LDS-DMA plan's estimate against the general family at 100 TFLOP/s (an operand on 2-byte gathers) or 600.
// several contracted modes and the fastest one fills less than 70 % of its K-tiles (the sweep mask of the LDS-DMA kernels keeps such a
// problem, plan_contraction.cpp h16_sweep_ragged, at that efficiency)
static bool h16_sweep_waste(const ContractionView& v) {
    if (v.K.size() < 2) return false;
    const int64_t e0 = v.K.front().extent;
    return e0 % 64 != 0 && (double)e0 < 0.7 * 64.0 * (double)((e0 + 63) / 64);
}
// fp32: what the plan that takes the operands as they lie will cost, when it is NOT on the LDS-DMA ring kernels (0: it is, or nothing to
// compare) — the cost model's estimate of the register-staged kernels, corrected by what they measure on the shapes of
// profiles/r06zzb_sweep_shapes_f32.jsonl: x 1.15 with 16-byte lanes (422 / 2103 / 170 us modelled, 498 / 2333 / 204 measured), x 2.5 when an
// operand is gathered element by element (390 / 265 / 1346 modelled, 1064 / 552 / 5865 measured)
static double f32_direct_estimate_us(const ContractionView& v, const std::vector<ContractionChoice>& ch) {
    if (v.dtype != HIP_R_32F || v.wide || ch.empty() || ch[0].family != 0) return 0.0;
    const GettKernelInfo* k = kernel_info(0, ch[0].kernel);
    if (k == nullptr || k->fragPartials) return 0.0;
    return ch[0].estimateUs * ((v.layA == LAY_S || v.layB == LAY_S) ? 2.5 : 1.15);
}
// fp64: what the general family costs when the direct plan gathers single elements (V = 1: 'ijk,lkj->il' 30 TFLOP/s, the larger 'mlik' case
// 15 — profiles/r06zzi_sweep_shapes_f64.jsonl); 0 when it stages 16-byte units (nothing to gain from a copy)
// complex64 likewise (8 real flops per multiply-add): 103 / 58 TFLOP/s on those two shapes at V = 1 (profiles/r06zzm_sweep_shapes_c64_before.jsonl)
static double f64_direct_estimate_us(const ContractionView& v, const ContractionChoice& gc) {
    if ((v.dtype != HIP_R_64F && v.dtype != HIP_C_32F) || v.wide || gc.family != 2) return 0.0;
    const GettKernelInfo* k = kernel_info(2, gc.kernel);
    if (k == nullptr || k->vec >= 2) return 0.0;
    const double mnk = (double)v.totL * (double)v.totM * (double)v.totN * (double)v.totK;
    return (v.dtype == HIP_C_32F ? 8.0 * mnk / 75e12 : 2.0 * mnk / 22e12) * 1e6 + 8.0;
}
// set while the inner contraction of a repacked plan is estimated / planned: the temporaries are final, no second round of copies
thread_local bool t_inRepack = false;

// ---- reduced-precision compute descriptors on fp32 and complex64 data (kernels/gett_gen_f32x.inc, gett_gen_c32x.inc) ------------
// COMPUTE_DESC_16F / _16BF / _TF32 on a contraction whose tensors are all real fp32 with fp32 scalars — or all complex64 with
// complex-float scalars — PERMIT products of rounded operands (fp16, bf16, three bf16 products of a hi / lo split; complex: each of the
// four real products of a complex one); the fp32 / complex64 kernels stay a legal answer.  Returns the general family's element for the
// descriptor, or -1 when the contraction is not of that kind.
static int f32x_elem_of(const cutensorOperationDescriptor& d) {
    if (d.kind != OpKind::Contraction || d.compute == nullptr || (d.scalarType != HIP_R_32F && d.scalarType != HIP_C_32F)) return -1;
    for (const TensorUse* t : {&d.A, &d.B, &d.C, &d.D})
        if (t->present && t->desc.dtype != d.scalarType) return -1;
    const bool cplx = d.scalarType == HIP_C_32F;
    switch (d.compute->id) {
        case 0:  return cplx ? GEN_C32_F16 : GEN_F32_F16;
        case 1:  return cplx ? GEN_C32_BF16 : GEN_F32_BF16;
        case 2:  return cplx ? GEN_C32_BF16X3 : GEN_F32_BF16X3;
        default: return -1;
    }
}
static const char* f32x_desc_name(int elem) {
    return (elem == GEN_F32_F16 || elem == GEN_C32_F16) ? "16F" : (elem == GEN_F32_BF16 || elem == GEN_C32_BF16) ? "16BF" : "TF32";
}
// CUTENSOR_AMD_F32X (test-hooks flavour): "force" — the reduced-precision kernels whenever the descriptor permits them; "0" — never
static int f32x_switch() {
    const char* e = CTAMD_HOOK_ENV("CUTENSOR_AMD_F32X");
    return (e == nullptr) ? 0 : (e[0] == 'f') ? 1 : (e[0] == '0') ? -1 : 0;
}
// Whether a plan for view `v` (fp32 or complex64 data, descriptor element `elem`) takes the reduced-precision kernels: `g` is their
// choice.  The full-precision side is `ch32`, the ranked fp32 candidates (best first), for fp32 data; for complex64 data (`ch32` is not
// read) it is the complex64 plan pick_gen_choice gives the same view, at its measured rate — both sides from
// gen_c32_measured_estimate_us (plan_contraction.cpp): one formula.  ONE rule for both: by the model, only problems it can place —
// 16-byte loads on both operands, no split-K on either side (the headline einsum's class stays on the split-K kernels), at least one
// output tile per CU, and an estimate below 0.8 x the full-precision plan's.  `note` says which side won and on what numbers (the
// CUTENSOR_LOG_LEVEL plan line).
static bool f32x_decide(const ContractionView& v, int elem, uint64_t wsLimit, int numCUs, bool explicitPick,
                        const std::vector<ContractionChoice>& ch32, ContractionChoice& g, std::string& note) {
    const int sw = f32x_switch();
    char buf[256];
    if (elem < 0 || v.wide || explicitPick || t_inRepack || sw < 0) return false;
    const bool cplx = gen_elem_is_c32x(elem);
    const char* full = cplx ? "complex64" : "fp32";
    if (!pick_gen_choice(v, wsLimit, numCUs, g, elem)) {
        note = std::string("no reduced-precision kernel for this view -> ") + full + " kernels";
        return false;
    }
    double t32 = -1.0;
    uint32_t split32 = 1;
    if (cplx) {
        ContractionChoice g32;
        if (pick_gen_choice(v, wsLimit, numCUs, g32)) { t32 = gen_c32_measured_estimate_us(v, g32, numCUs); split32 = g32.splitK; }
    } else if (!ch32.empty() && ch32[0].family == 0 && ch32[0].kernel >= 0) {
        t32 = ch32[0].estimateUs;
        split32 = ch32[0].splitK;
    }
    if (sw > 0) {
        std::snprintf(buf, sizeof buf, "reduced-precision kernels forced (model %.1f us, %s plan %.1f us)", g.estimateUs, full, t32);
        note = buf;
        return true;
    }
    const GettKernelInfo& k = *kernel_info(2, g.kernel);
    const double tiles = std::ceil((double)v.totM / k.bm) * std::ceil((double)v.totN / k.bn) * (double)v.totL;
    const char* why = nullptr;
    if (t32 < 0.0) why = "no full-precision MFMA plan to compare with";
    else if (k.vec != (cplx ? 2 : 4)) why = "element gathers";
    else if (g.splitK > 1 || split32 > 1) why = "split-K problem";
    else if (tiles < (double)numCUs) why = "fewer output tiles than CUs";
    else if (!(g.estimateUs < 0.8 * t32)) why = "model sees no gain";
    std::snprintf(buf, sizeof buf, "%s %s (model: reduced-precision %.1f us, %s plan %.1f us)%s%s", why ? full : "reduced-precision", why ? "kernels kept" : "kernels",
                  g.estimateUs, full, t32, why ? ": " : "", why ? why : "");
    note = buf;
    return why == nullptr;
}
// ---- COMPUTE_DESC_32F on fp64 / complex128 data (kernels/gett_gen_f64x.inc) ----------------------------------------------------
thread_local int t_f64xOff = 0;
// On a contraction whose tensors are all real fp64 (all complex128) with double (complex double) scalars the descriptor PERMITS
// products of operands rounded once to fp32, on the fp32 MFMA; the fp64 kernels stay a legal answer.  Returns the general family's
// element for the descriptor, or -1 when the contraction is not of that kind.
int f64x_elem_of(const cutensorOperationDescriptor& d) {
    if (d.kind != OpKind::Contraction || d.compute == nullptr || d.compute->id != 4) return -1;
    const hipDataType t = d.A.desc.dtype;
    if ((t != HIP_R_64F && t != HIP_C_64F) || d.scalarType != t) return -1;
    for (const TensorUse* u : {&d.A, &d.B, &d.C, &d.D})
        if (u->present && u->desc.dtype != t) return -1;
    return t == HIP_R_64F ? GEN_F64_F32 : GEN_C64_C32;
}
// CUTENSOR_AMD_F64X (test-hooks flavour): "force" — the single-precision kernels whenever the descriptor permits them; "0" — never
static int f64x_switch() {
    const char* e = CTAMD_HOOK_ENV("CUTENSOR_AMD_F64X");
    return (e == nullptr) ? 0 : (e[0] == 'f') ? 1 : (e[0] == '0') ? -1 : 0;
}
// Whether a plan for view `v` (fp64 / complex128 data, descriptor element `elem`) takes the single-precision kernels: `g` is their
// choice, compared with the fp64 plan pick_gen_choice gives the same view.  By the model, only problems it can place: 16-byte loads on
// both operands, no split-K on either side, at least one output tile per CU, and an estimate below 0.8 x the fp64 plan's — both from
// gen_f64_measured_estimate_us (plan_contraction.cpp): one formula, each side at its measured rate.  `note` says
// which side won and on what numbers (the CUTENSOR_LOG_LEVEL plan line).
static bool f64x_decide(const ContractionView& v, int elem, uint64_t wsLimit, int numCUs, bool explicitPick, ContractionChoice& g, std::string& note) {
    const int sw = f64x_switch();
    char buf[256];
    if (elem < 0 || v.wide || explicitPick || t_inRepack || t_f64xOff > 0 || sw < 0) return false;
    if (!pick_gen_choice(v, wsLimit, numCUs, g, elem)) { note = "no single-precision kernel for this view -> fp64 kernels"; return false; }
    ContractionChoice g64;
    const bool have64 = pick_gen_choice(v, wsLimit, numCUs, g64);
    const double t64 = have64 ? gen_f64_measured_estimate_us(v, g64, numCUs) : -1.0;
    if (sw > 0) {
        std::snprintf(buf, sizeof buf, "single-precision kernels forced (model %.1f us, fp64 plan %.1f us)", g.estimateUs, t64);
        note = buf;
        return true;
    }
    const GettKernelInfo& k = *kernel_info(2, g.kernel);
    const double tiles = std::ceil((double)v.totM / k.bm) * std::ceil((double)v.totN / k.bn) * (double)v.totL;
    const char* why = nullptr;
    if (!have64) why = "no fp64 MFMA plan to compare with";
    else if (elem == GEN_F64_F32 && k.vec != 2) why = "element gathers";
    else if (g.splitK > 1 || g64.splitK > 1) why = "split-K problem";
    else if (tiles < (double)numCUs) why = "fewer output tiles than CUs";
    else if (!(g.estimateUs < 0.8 * t64)) why = "model sees no gain";
    std::snprintf(buf, sizeof buf, "%s (model: single-precision %.1f us, fp64 plan %.1f us)%s%s", why ? "fp64 kernels kept" : "single-precision kernels",
                  g.estimateUs, t64, why ? ": " : "", why ? why : "");
    note = buf;
    return why == nullptr;
}
// tDirectUs: the estimate of the plan that takes the operands as they lie, when the LDS-DMA family has one (sweeps of a short ragged contracted
// mode waste most of every K-tile: 'abcd,dcbe->ae' with d = 16 keeps 16 of 64 k) — negative: the general family's model above.
static bool plan_repack(const cutensorHandle* handle, const cutensorOperationDescriptor& desc, const ContractionView& v, uint64_t wsLimit, double tDirectUs, TwoStepSplit& out) {
    const bool f32 = v.dtype == HIP_R_32F, c32 = v.dtype == HIP_C_32F, f64 = v.dtype == HIP_R_64F || c32;   // (f64: the general family's wide elements)
    if (t_inRepack || v.wide || (v.dtype != HIP_R_16BF && v.dtype != HIP_R_16F && !f32 && !f64) || v.K.empty()) return false;
    const double es = (double)dtype_size(v.dtype);
    if (desc.A.op != CUTENSOR_OP_IDENTITY || desc.B.op != CUTENSOR_OP_IDENTITY) return false;
    auto has = [](const std::vector<int32_t>& m, int32_t l) { return std::find(m.begin(), m.end(), l) != m.end(); };
    auto stride_of = [](const TensorUse& T, int32_t l) -> int64_t {
        for (size_t i = 0; i < T.modes.size(); ++i) if (T.modes[i] == l) return T.desc.stride[i];
        return 0;
    };
    // freeMajor: the FREE modes fastest (D's order), then the contracted modes in X's own order (a plain matrix transpose when they are
    // adjacent in X): the temporary is free-contiguous, and a free-contiguous operand takes ANY fastest contracted extent under the sweep
    // mask — the way out for sweeps that end in partial 16-byte units ('abcd,dcbe->ae' with d = 50)
    auto pack = [&](const TensorUse& X, const TensorUse& other, bool freeMajor, cutensorOperationDescriptor& perm, TensorUse& kept, uint64_t& bytes, double& copyUs) {
        struct Km { int32_t label; int64_t extent, so; };
        std::vector<Km> k;
        for (size_t i = 0; i < X.modes.size(); ++i) {
            const int32_t l = X.modes[i];
            const bool inO = has(other.modes, l), inD = has(desc.D.modes, l);
            if (!inO && !inD) return false;                                 // (an extent-1 mode nothing else carries: leave the descriptor alone)
            if (inO && !inD) k.push_back(Km{l, X.desc.extent[i], std::llabs(freeMajor ? X.desc.stride[i] : stride_of(other, l))});
        }
        std::stable_sort(k.begin(), k.end(), [](const Km& a, const Km& b) { return a.so < b.so; });
        PackedTemporary t(X);
        auto push = [&](int32_t l, int64_t e) { t.push(l, e); };
        if (!freeMajor) for (const Km& m : k) push(m.label, m.extent);
        for (int pass = 0; pass < 2; ++pass) {                              // free modes in D's order, then the batch modes
            if (freeMajor && pass == 1) for (const Km& m : k) push(m.label, m.extent);
            for (int32_t l : desc.D.modes) {
                if (!has(X.modes, l) || (has(other.modes, l) ? 1 : 0) != pass) continue;
                for (size_t i = 0; i < X.modes.size(); ++i) if (X.modes[i] == l) push(l, X.desc.extent[i]);
            }
        }
        if (t.use.modes.size() != X.modes.size()) return false;
        kept = t.use;
        bytes = t.bytes();
        perm = cutensorOperationDescriptor{};
        perm.kind = OpKind::Permutation;
        perm.A = X;
        perm.D = kept; perm.D.op = CUTENSOR_OP_IDENTITY;
        perm.compute = desc.compute;
        perm.scalarType = desc.scalarType;
        perm.movedBytes = 2.0 * (double)bytes;
        // what the copy costs, by the kernel the element-wise planner gives it: the tiled kernels move whole tiles at ~4 TB/s (a tile mode
        // much shorter than its tile pays for the padding), the element-gather kernel ~15 G elements per second (measured, round 6:
        // 13 MB of bf16 from [d = 50, c, b, a] to [b, c, d, a] in 380 us)
        EwPlan ep;
        if (plan_elementwise(perm, ep, nullptr) != CUTENSOR_STATUS_SUCCESS) return false;
        const double elems = (double)t.elems;
        if (ep.variant == EW_TRANSPOSE) {
            // (rows of a tile past the end of a mode are skipped, not moved: the padding costs about a third of live data — 'jkl -> kjl'
            // with 16 x 72 of every 64 x 128 tile pair live, 9.4 MB, measured ~15 us)
            const double padded = (double)ep.p.tiles0 * ep.p.tile0 * (double)ep.p.tiles1 * ep.p.tile1 * (double)ep.p.rest.total;
            copyUs = 4.0 + 2.0 * es * (elems + 0.35 * (padded - elems)) / 4e6;
        }
        else if (ep.variant == EW_ROWCOPY || ep.variant == EW_BLOCK) copyUs = 4.0 + 2.0 * es * elems / 4e6;
        else if (ep.variant == EW_TRANSPOSE_ANY) copyUs = 4.0 + 2.0 * es * elems / 2e6;
        else copyUs = 4.0 + elems / 15e3;
        return true;
    };
    const bool slowA = (v.swapped ? v.layB : v.layA) == LAY_S, slowB = (v.swapped ? v.layA : v.layB) == LAY_S;   // the user's A is kernel-B when swapped
    const double flops = 2.0 * (double)v.totL * (double)v.totM * (double)v.totN * (double)v.totK;
    const double tGeneral = tDirectUs >= 0.0 ? tDirectUs : flops / ((slowA || slowB) ? 100e12 : 400e12) * 1e6 + 8.0;
    // candidates: A, B or both copied, each with its contracted or its free modes fastest — with both K-major, the temporaries share one
    // order of the contracted modes, which then fuse into a single one (nothing ragged but the end of K).  The fastest one by the model,
    // if it beats the direct plan by a fifth.
    // (CUTENSOR_AMD_REPACK=f, hooks flavour: whenever the temporaries fit — the fuzzers' and the small parity cases' way onto this path)
    const bool forced = CTAMD_HOOK_ENV_IS("CUTENSOR_AMD_REPACK", 'f');
    double best = 1e30;
    for (int attempt = 1; attempt < 9; ++attempt) {                         // per operand: 0 = as it lies, 1 = contracted modes fastest, 2 = free modes fastest
        const int howA = attempt % 3, howB = attempt / 3;
        const bool doA = howA != 0, doB = howB != 0;
        // (every combination is tried: an operand the kernels cannot stage as it lies may become stageable once the OTHER one is copied —
        // A[d = 50, c, b, a] is K-contiguous in the fused mode (d, c, b) as soon as B holds the contracted modes in that order)
        TwoStepSplit r;
        TensorUse keptA, keptB;
        // the order of the contracted modes follows the OTHER operand as it will be contracted: with both repacked, B follows A's temporary
        double usA = 0.0, usB = 0.0;
        if (doA && !pack(desc.A, desc.B, howA == 2, r.stepA, keptA, r.bytesA, usA)) continue;
        if (doB && !pack(desc.B, doA ? keptA : desc.A, howB == 2, r.stepB, keptB, r.bytesB, usB)) continue;
        r.hasA = doA; r.hasB = doB;
        r.inner = desc;
        if (doA) r.inner.A = keptA;
        if (doB) r.inner.B = keptB;
        const uint64_t temps = TwoStepLayout(r.bytesA, r.bytesB).offW;
        if (temps > wsLimit) continue;
        ContractionView vi;
        ContractionChoice hc;
        if (build_contraction_view(r.inner, vi, nullptr) != CUTENSOR_STATUS_SUCCESS || vi.wide) continue;
        if (f64) {
            // fp64 (general MFMA family, gett_gen.inc): the temporaries must give both operands 16-byte units (V = 2) where the direct plan
            // gathers single elements; the family's rates on the shapes of profiles/r06zzi_sweep_shapes_f64.jsonl: 52-59 TFLOP/s at V = 2
            const GettKernelInfo* k = pick_gen_choice(vi, wsLimit - temps, handle->numCUs, hc) ? kernel_info(2, hc.kernel) : nullptr;
            if (k == nullptr || k->vec < 2) continue;
            hc.estimateUs = (c32 ? 4.0 * flops / 124e12 : flops / 55e12) * 1e6 + 8.0;   // (complex64 at V = 2: 124 TFLOP/s of real flops, r06zzm)
        } else if (f32) {
            // fp32: the temporaries must put the problem on the LDS-DMA ring kernels (gett_f32_stream.hip: whole 32-deep K-tiles in the
            // fastest contracted mode, or one ragged contracted mode)
            const std::vector<ContractionChoice> ci = rank_contraction_choices(vi, wsLimit - temps, handle->numCUs, false);
            const GettKernelInfo* k = (ci.empty() || ci[0].family != 0) ? nullptr : kernel_info(0, ci[0].kernel);
            if (k == nullptr || (!forced && !k->fragPartials)) continue;
            hc = ci[0];
        } else if (!pick_h16_choice(vi, wsLimit - temps, handle->numCUs, hc)) continue;
        const double tCopies = usA + usB;
        if (tCopies + hc.estimateUs < best) { best = tCopies + hc.estimateUs; out = r; }
    }
    if (best >= 1e30) return false;
    return forced || best < 0.8 * tGeneral;
}

// pointer alignment the offset operands of a peeled contraction still have
static void peel_fix_alignment(cutensorOperationDescriptor& inner, const std::vector<PeelMode>& peel) {
    auto fix = [&](TensorUse& t, int which) {
        const int64_t es = (int64_t)dtype_size(t.desc.dtype);      // each tensor's own (a mixed contraction's real input: 8 bytes)
        uint32_t a = t.desc.alignment;
        for (const PeelMode& pm : peel) {
            const int64_t s = which == 0 ? pm.sA : which == 1 ? pm.sB : which == 2 ? pm.sC : pm.sD;
            while (a > (uint32_t)es && ((s * es) % (int64_t)a) != 0) a >>= 1;
        }
        t.desc.alignment = std::max<uint32_t>(a, (uint32_t)es);
    };
    fix(inner.A, 0); fix(inner.B, 1); fix(inner.C, 2); fix(inner.D, 3);
}

// ---- the routes of a contraction, in the order they are tried -------------------------------------------------------------------
// The plan builders (create_plan.cpp, build_contraction) and the workspace estimate (estimate_contraction below) walk the same functions on
// the same PlanRequest: the operands reduced over their lone modes first (split_lone_modes), then the view, then route_peeled,
// route_mode_table, rank_tiled_candidates, route_repack, and what is left is a tiled plan or the simple kernel (route_tiled).  Every
// condition on the way, and every test-hook switch that moves a problem from one route to another, is read here and nowhere else.

// any experiment knob that changes what cutensorCreatePlan decides: the memo stands aside while one is set
bool plan_env_override() {
    return CTAMD_HOOK_ENV("CUTENSOR_AMD_FORCE") || CTAMD_HOOK_ENV("CUTENSOR_AMD_XCD_BALANCE") || CTAMD_HOOK_ENV("CUTENSOR_AMD_FUSED_FOLD") ||
           CTAMD_HOOK_ENV("CUTENSOR_AMD_H16_TRANSPOSE_T1") || CTAMD_HOOK_ENV("CUTENSOR_AMD_NT") || CTAMD_HOOK_ENV("CUTENSOR_AMD_H16_WAVES") || CTAMD_HOOK_ENV("CUTENSOR_AMD_H16_SPLITK") ||
           CTAMD_HOOK_ENV("CUTENSOR_AMD_KORDER") || CTAMD_HOOK_ENV("CUTENSOR_AMD_ABLATION") || CTAMD_HOOK_ENV("CUTENSOR_AMD_PEEL") || CTAMD_HOOK_ENV("CUTENSOR_AMD_GEN") ||
           CTAMD_HOOK_ENV("CUTENSOR_AMD_REPACK") || CTAMD_HOOK_ENV("CUTENSOR_AMD_EW_ANY") || CTAMD_HOOK_ENV("CUTENSOR_AMD_F32X") ||
           CTAMD_HOOK_ENV("CUTENSOR_AMD_F64X") || CTAMD_HOOK_ENV("CUTENSOR_AMD_F32_SPLITK") || CTAMD_HOOK_ENV("CUTENSOR_AMD_EW_TABLE");
}
// CUTENSOR_AMD_GEN=0 (hooks flavour): never the general MFMA family
static bool gen_family_off() { return CTAMD_HOOK_ENV_IS("CUTENSOR_AMD_GEN", '0'); }

// too many unfusable modes in a group for the tiled kernels (v.wide): peel the smallest ones into a host loop if that takes at most
// kMaxPeelLaunches launches (peel_wide_contraction); `inner` is the problem of one launch
bool route_peeled(const PlanRequest& rq, const ContractionView& v, cutensorOperationDescriptor& inner, std::vector<PeelMode>& peel) {
    if (!v.wide || CTAMD_HOOK_ENV_IS("CUTENSOR_AMD_PEEL", '0') || !peel_wide_contraction(rq.desc, inner, peel)) return false;
    peel_fix_alignment(inner, peel);
    return true;
}
// the mode-table kernel: views the tiled kernels cannot describe, and complex data off the general MFMA family — it only multiplies
// there or on the mode-table kernel (complex scalars of the data's type); such a view turns wide here
bool route_mode_table(const PlanRequest& rq, ContractionView& v, bool accumulate64) {
    const bool cplx = v.dtype == HIP_C_32F || v.dtype == HIP_C_64F;
    if (cplx && (gen_family_off() || rq.desc.scalarType != v.dtype || (v.dtype == HIP_C_32F && accumulate64))) v.wide = true;
    return v.wide;
}
TiledRoute rank_tiled_candidates(const PlanRequest& rq, const ContractionView& v, bool accumulate64) {
    const cutensorOperationDescriptor& desc = rq.desc;
    const int numCUs = rq.handle->numCUs;
    TiledRoute r;
    r.mfmaPath = v.dtype == HIP_R_32F && !accumulate64;
    r.h16Path = !r.mfmaPath && !accumulate64 && desc.scalarType == HIP_R_32F && (v.dtype == HIP_R_16BF || v.dtype == HIP_R_16F);
    // general MFMA family: 16-bit shapes the aligned kernels refuse, fp64 (double scalars), complex (complex scalars)
    r.genPath = r.h16Path || (v.dtype == HIP_R_64F && desc.scalarType == HIP_R_64F) ||
                (v.dtype == HIP_C_32F && desc.scalarType == HIP_C_32F && !accumulate64) ||
                (v.dtype == HIP_C_64F && desc.scalarType == HIP_C_64F);
    if (r.mfmaPath) r.ch = rank_contraction_choices(v, rq.wsLimit, numCUs, rq.pr.operandsStreamed != 0);
    else if (r.h16Path && !CTAMD_HOOK_ENV_IS("CUTENSOR_AMD_GEN", 'f'))   // "force" (measurement): the general family also where the aligned 16-bit kernels apply
        r.ch = rank_h16_choices(v, rq.wsLimit, numCUs);
    if (r.mfmaPath && desc.scalarType == HIP_R_32F && !names_candidate(rq.pr) && !CTAMD_HOOK_ENV("CUTENSOR_AMD_KORDER"))
        r.tDirectUs = f32_direct_estimate_us(v, r.ch);
    const bool explicitPick = names_candidate_or_tunes(rq.pr);
    if (r.mfmaPath) {
        // a reduced-precision compute descriptor: the bf16 / fp16-rate kernels when the model (or CUTENSOR_AMD_F32X=force) says so.
        // They take the operands as they lie (no repack pre-pass); a caller who names a candidate addresses the fp32 list as ever.
        const int xe = f32x_elem_of(desc);
        ContractionChoice gx;
        std::string note;
        if (xe >= 0 && f32x_decide(v, xe, rq.wsLimit, numCUs, explicitPick, r.ch, gx, note)) {
            r.ch.assign(1, gx);
            r.tDirectUs = 0.0;
        }
        if (xe >= 0 && !note.empty()) r.notes.push_back(std::string("plan: fp32 contraction, compute descriptor ") + f32x_desc_name(xe) + ": " + note);
    }
    if (r.genPath && !r.h16Path) {
        // COMPUTE_DESC_32F on fp64 / complex128 data: the fp32-rate kernels when the model (or CUTENSOR_AMD_F64X=force) says so.  They take
        // the operands as they lie (no repack pre-pass); a caller who names a candidate gets the fp64 plan as ever.
        const int xe = f64x_elem_of(desc);
        ContractionChoice gx;
        std::string note;
        if (xe >= 0 && !gen_family_off() && f64x_decide(v, xe, rq.wsLimit, numCUs, explicitPick, gx, note)) r.ch.assign(1, gx);
        if (xe >= 0 && !note.empty()) r.notes.push_back(std::string("plan: ") + (xe == GEN_F64_F32 ? "fp64" : "complex128") + " contraction, compute descriptor 32F: " + note);
        // a reduced-precision compute descriptor on complex64 data (16BF / 16F / TF32): the 16-bit-rate kernels when the model (or
        // CUTENSOR_AMD_F32X=force) says so, on the operands as they lie; a caller who names a candidate gets the complex64 plan as ever
        const int ce = (v.dtype == HIP_C_32F && !gen_family_off()) ? f32x_elem_of(desc) : -1;
        std::string cnote;
        if (ce >= 0 && f32x_decide(v, ce, rq.wsLimit, numCUs, explicitPick, r.ch, gx, cnote)) r.ch.assign(1, gx);
        if (ce >= 0 && !cnote.empty()) r.notes.push_back(std::string("plan: complex64 contraction, compute descriptor ") + f32x_desc_name(ce) + ": " + cnote);
        if (!r.ch.empty()) return r;
    }
    if ((v.dtype == HIP_R_64F || v.dtype == HIP_C_32F) && desc.scalarType == v.dtype && r.genPath && r.ch.empty()) {   // fp64 / complex64 on element gathers (plan_repack)
        ContractionChoice g64;
        if (pick_gen_choice(v, rq.wsLimit, numCUs, g64)) r.tDirectUs = f64_direct_estimate_us(v, g64);
    }
    return r;
}
// The LDS-DMA kernels refuse the operands as they lie (or would spend most of every K-tile on the padding of a short ragged contracted
// mode), or fp32 / fp64 / complex64 data is off its fast kernels: copy operands into packed temporaries first when that pays (plan_repack)
bool route_repack(const PlanRequest& rq, const ContractionView& v, const TiledRoute& r, TwoStepSplit& rs) {
    const bool h16Refused = r.h16Path && (r.ch.empty() || h16_sweep_waste(v)) && !CTAMD_HOOK_ENV("CUTENSOR_AMD_GEN") && !CTAMD_HOOK_ENV("CUTENSOR_AMD_H16_WAVES");
    if (!(h16Refused || r.tDirectUs > 0.0) || names_candidate(rq.pr) ||      // (a caller who names a candidate gets that candidate)
        CTAMD_HOOK_ENV_IS("CUTENSOR_AMD_REPACK", '0'))
        return false;
    return plan_repack(rq.handle, rq.desc, v, rq.wsLimit, r.tDirectUs > 0.0 ? r.tDirectUs : r.ch.empty() ? -1.0 : r.ch[0].estimateUs, rs);
}
// what is left: the ranked candidates, else the one choice of the general family; r.ch stays empty for the simple kernel
void route_tiled(const PlanRequest& rq, const ContractionView& v, TiledRoute& r) {
    ContractionChoice g;
    if (r.ch.empty() && r.genPath && !gen_family_off() && pick_gen_choice(v, rq.wsLimit, rq.handle->numCUs, g)) r.ch.push_back(g);
}

// cutensorEstimateWorkspaceSize of a contraction without lone modes: the route at the preference's cap (rq.wsLimit), added up.  Two
// routes can still fall through to the next one after their sub-plans are built (build_peeled: the inner plan is not one launch;
// build_repack: the inner plan leaves the family); the estimate prices the first proposal there.
cutensorStatus_t estimate_contraction(const PlanRequest& rq, cutensorWorksizePreference_t workspacePref, uint64_t* estimate) {
    ContractionView v;
    const cutensorStatus_t st = build_contraction_view(rq.desc, v, nullptr);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    const bool accumulate64 = accumulates_in_fp64(rq.desc);
    auto inner_estimate = [&](cutensorOperationDescriptor& d, uint64_t* w) { return cutensorEstimateWorkspaceSize(rq.handle, &d, rq.pref, workspacePref, w); };
    cutensorOperationDescriptor inner;
    std::vector<PeelMode> peel;
    if (route_peeled(rq, v, inner, peel)) return inner_estimate(inner, estimate);   // what its inner, tiled problem wants
    if (route_mode_table(rq, v, accumulate64)) return CUTENSOR_STATUS_SUCCESS;
    TiledRoute r = rank_tiled_candidates(rq, v, accumulate64);
    TwoStepSplit rs;
    if (route_repack(rq, v, r, rs)) {   // the temporaries + what the inner contraction on them wants
        uint64_t wI = 0;
        RepackScope scope;
        const cutensorStatus_t sti = inner_estimate(rs.inner, &wI);
        if (sti == CUTENSOR_STATUS_SUCCESS) *estimate = TwoStepLayout(rs.bytesA, rs.bytesB).offW + wI;
        return sti;
    }
    route_tiled(rq, v, r);
    // the fp32 ranked list: the largest workspace any of the best four candidates would like to have (room for the candidate autotuning
    // or the plan cache settles on); every other route has one choice
    const size_t considered = (!r.ch.empty() && r.ch[0].family == 0) ? 4 : 1;
    for (size_t i = 0; i < r.ch.size() && i < considered; ++i) *estimate = std::max(*estimate, r.ch[i].workspace);
    return CUTENSOR_STATUS_SUCCESS;
}

}  // namespace ctamd
