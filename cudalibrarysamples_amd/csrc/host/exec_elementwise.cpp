// exec_elementwise.cpp — the element-wise and reduction family behind the C ABI: cutensorPermute, cutensorElementwiseBinaryExecute,
// cutensorElementwiseTrinaryExecute, cutensorReduce and their arms of ctamdDescribePlan.  Every launch of an element-wise plan, whatever
// its form and data type, goes through run_elementwise; the trinary forms are decoded once (trinary_roles) for the executor and the
// description alike.  Each entry point cites the reference call site it serves.
#include <cstdio>

#include <hip/hip_runtime.h>

#include "internal.hpp"

using namespace ctamd;

namespace ctamd {

// a zero gamma drops the C term only for ADD (alpha perm(A) + 0): MUL / MAX / MIN still need it
static bool reads_c(const EwPlan& ew, CxScalar gamma) {
    return ew.usesC && (gamma.re != 0.0 || gamma.im != 0.0 || (ew.p.opAC != 0 && ew.p.opAC != CUTENSOR_OP_ADD));
}

// a plan on the mode table (elementwise_table.hip): the table by value, pointers and scalars written per launch
static hipError_t run_elementwise_table(const EwPlan& ew, hipDataType dtype, const EwCall& c, hipStream_t stream) {
    if (!ew.tab || c.X != nullptr || c.E != nullptr) return hipErrorInvalidValue;      // (the trinary planner never gets this variant)
    EwTable t = *ew.tab;
    t.A = c.A; t.D = c.D;
    t.C = reads_c(ew, c.gamma) ? c.C : nullptr;
    t.alpha64 = c.alpha.re; t.alphaIm = c.alpha.im;
    t.gamma64 = c.gamma.re; t.gammaIm = c.gamma.im;
    return launch_elementwise_table(t, (int)dtype, ew.tabGrid, stream);
}

hipError_t run_elementwise(const EwPlan& ew, hipDataType dtype, const EwCall& c, hipStream_t stream) {
    if (ew.on_table()) return run_elementwise_table(ew, dtype, c, stream);
    Ew2DParams p = ew.p;
    p.A = c.A; p.X = c.X; p.E = c.E; p.D = c.D;
    p.C = reads_c(ew, c.gamma) ? c.C : nullptr;
    p.alpha = (float)c.alpha.re; p.alpha64 = c.alpha.re; p.alphaIm = c.alpha.im;
    p.gamma = (float)c.gamma.re; p.gamma64 = c.gamma.re; p.gammaIm = c.gamma.im;
    p.xi = (float)c.xi.re; p.xi64 = c.xi.re;
    p.delta = (float)c.delta.re; p.delta64 = c.delta.re;
    // the block kernel moves elements and scales them, nothing else: under a unary operator the plan runs on the kernel its tiles were
    // laid out for (same variant in the description, as for an attached operand)
    const int variant = (ew.variant == EW_BLOCK && p.unA != 0) ? ew.blockFrom : ew.variant;
    if (ew.converts()) return launch_elementwise_convert(p, variant, (int)ew.dtypeA, (int)ew.dtypeD, stream);
    // complex data with an E or X operand: the kernels of elementwise.hip take neither (kernels/elementwise_trinary_cplx.hip)
    if ((dtype == HIP_C_32F || dtype == HIP_C_64F) && (c.X != nullptr || c.E != nullptr))
        return launch_elementwise_trinary_cplx(p, Ew3CplxExtras{c.xi.im, c.delta.im, ew.conjX, ew.conjE}, variant, (int)dtype, stream);
    return launch_elementwise(p, variant, (int)dtype, stream);
}

// What a trinary form (plan_elementwise_trinary) made of the caller's A and of the caller's B: the tile operand of the last pass, its
// second permuted operand X, the operand E that rides along with D's strides, or the input of pass 1
enum class EwRole { Tile, X, E, First };
struct EwRoles { EwRole a, b; };
static EwRoles trinary_roles(const EwTrinaryPlan& t) {
    if (t.bothPermuted) return {EwRole::Tile, EwRole::X};       // one pass, two tiles
    if (t.twoPass) return {EwRole::First, EwRole::Tile};        // D = alpha perm(A), then combined in place with beta perm(B)
    if (t.swapAB) return {EwRole::Tile, EwRole::E};             // E = B (has D's layout)
    return {EwRole::E, EwRole::Tile};                           // E = A
}

struct EwPass { const EwPlan* ew = nullptr; EwCall call; };
struct EwPasses { int n = 0; EwPass pass[2]; };                 // n = 0: called in place, and the plan has no single-launch form

// The launches of one trinary call, in order.  Two-pass form with C inside D's range (in-place use: C == D) and read by the last pass:
// pass 1 would overwrite it first, so ONE launch of the element-gather kernel runs instead (EwTrinaryPlan::gather) — a lane reads its
// element of C before it writes that element of D — with A on its tile path and B as X, the roles of the two-tile form.
static EwPasses trinary_passes(const EwTrinaryPlan& t, const void* A, const void* B, const void* C, void* D, CxScalar alpha, CxScalar beta,
                               CxScalar gamma) {
    EwPasses out;
    const uintptr_t c = reinterpret_cast<uintptr_t>(C), d = reinterpret_cast<uintptr_t>(D);
    const bool inPlace = t.twoPass && reads_c(t.last, gamma) && c < d + t.spanD && d < c + t.spanC;
    if (inPlace && !t.hasGather) return out;                    // (more unfusable modes than the single launch describes)
    const EwRoles r = inPlace ? EwRoles{EwRole::Tile, EwRole::X} : trinary_roles(t);
    EwCall first, last;
    first.D = last.D = D;
    last.C = C; last.gamma = gamma;
    auto put = [&](EwRole role, const void* ptr, CxScalar s) {
        switch (role) {
            case EwRole::Tile:  last.A = ptr; last.alpha = s; break;
            case EwRole::X:     last.X = ptr; last.xi = s; break;
            case EwRole::E:     last.E = ptr; last.delta = s; break;
            case EwRole::First: first.A = ptr; first.alpha = s; last.E = D; last.delta = CxScalar{1.0, 0.0}; break;   // in place, E = D
        }
    };
    put(r.a, A, alpha);
    put(r.b, B, beta);
    if (r.a == EwRole::First) out.pass[out.n++] = EwPass{&t.first, first};
    out.pass[out.n++] = EwPass{inPlace ? &t.gather : &t.last, last};
    return out;
}

// A plan whose operands carry a unary operator other than IDENTITY / CONJ: the closing '}' of the description in buf[0, n) becomes
// ,"unary":[opA, opB, opC]} (cutensorOperator_t values, IDENTITY where there is none).  Every other description stays as it is.
static int describe_unary(char* buf, size_t len, int n, int32_t a, int32_t b, int32_t c) {
    if ((a == 0 && b == 0 && c == 0) || n <= 0 || (size_t)n >= len || buf[n - 1] != '}') return n;
    auto code = [](int32_t u) { return u == 0 ? (int)CUTENSOR_OP_IDENTITY : (int)u; };
    return n - 1 + std::snprintf(buf + n - 1, len - (size_t)n + 1, ",\"unary\":[%d,%d,%d]}", code(a), code(b), code(c));
}

int describe_elementwise(const cutensorPlan& pl, char* buf, size_t len) {
    int n = 0;
    if (pl.kind == OpKind::Reduction && !pl.red.isPermutation && pl.red.variant == RED_TABLE) {
        // the fields of every reduction plan, then the mode table's: the modes of the view (kept + reduced) and the kernel
        n = std::snprintf(buf, len, "{\"op\":\"reduction\",\"variant\":%d,\"kept\":%u,\"red\":%u,\"splitR\":%u,\"redPerSplit\":%u,\"rowAny\":0,\"workspace\":%llu,"
                          "\"modes\":%u,\"keptModes\":%u,\"kname\":\"reduce_table_kernel\"}",
                          pl.red.variant, pl.red.p.kept.total, pl.red.p.red.total, pl.red.p.splitR, pl.red.p.redPerSplit,
                          (unsigned long long)pl.requiredWorkspace, pl.red.tab->nModes, pl.red.tab->nKept);
        n = describe_unary(buf, len, n, pl.red.p.unA, 0, pl.red.p.unC);
    } else if (pl.kind == OpKind::Reduction && !pl.red.isPermutation) {
        n = std::snprintf(buf, len, "{\"op\":\"reduction\",\"variant\":%d,\"kept\":%u,\"red\":%u,\"splitR\":%u,\"redPerSplit\":%u,\"rowAny\":%u,\"workspace\":%llu}",
                          pl.red.variant, pl.red.p.kept.total, pl.red.p.red.total, pl.red.p.splitR, pl.red.p.redPerSplit,
                          pl.red.p.rowAny, (unsigned long long)pl.requiredWorkspace);
        n = describe_unary(buf, len, n, pl.red.p.unA, 0, pl.red.p.unC);
    } else if (pl.kind == OpKind::ElementwiseTrinary) {
        // the three forms (plan_elementwise_trinary): one pass with E, one pass with two tiles, two passes (variant_first: pass 1's kernel;
        // variant_inplace: the single launch that replaces both passes when C overlaps D, -1 if there is none).  "op" stays "elementwise",
        // as for every plan of the element-wise family; "form" tells the trinary plans from the others
        const EwTrinaryPlan& t = pl.ew3;
        n = std::snprintf(buf, len, "{\"op\":\"elementwise\",\"form\":\"trinary\",\"passes\":%d,\"bothPermuted\":%d,\"swapAB\":%d,\"variant\":%d,\"variant_first\":%d,"
                          "\"variant_inplace\":%d,\"E0\":%u,\"E1\":%u,\"rest\":%u,\"blocks\":%u,\"tile0\":%u}",
                          t.twoPass ? 2 : 1, (int)t.bothPermuted, (int)t.swapAB, t.last.variant, t.twoPass ? t.first.variant : -1,
                          t.hasGather ? t.gather.variant : -1, t.last.p.E0, t.last.p.E1, t.last.p.rest.total, t.last.p.nBlocks, t.last.p.tile0);
        // each operand's operator and (complex plans) conjugation, read back from the role its form gave it
        const Ew2DParams& q = t.last.p;
        auto unary = [&](EwRole r) { return r == EwRole::Tile ? q.unA : r == EwRole::X ? q.unX : r == EwRole::E ? q.unE : t.first.p.unA; };
        auto conj = [&](EwRole r) { return r == EwRole::Tile ? q.conjA : r == EwRole::X ? t.last.conjX : r == EwRole::E ? t.last.conjE : t.first.p.conjA; };
        const EwRoles r = trinary_roles(t);
        n = describe_unary(buf, len, n, unary(r.a), unary(r.b), q.unC);
        if ((pl.dtype == HIP_C_32F || pl.dtype == HIP_C_64F) && n > 1 && (size_t)n < len && buf[n - 1] == '}')
            n = n - 1 + std::snprintf(buf + n - 1, len - (size_t)n + 1, ",\"conj\":[%d,%d,%d]}", (int)conj(r.a), (int)conj(r.b), (int)q.conjC);
    } else {
        const EwPlan& e = (pl.kind == OpKind::Reduction) ? pl.red.perm : pl.ew;
        if (e.on_table()) {
            // a plan on the mode table: "modes" of the view, "tile" = [positions of a tile, modes taken from A's side, from D's side]
            // (zeros on the gather kernel), "blocks" = tiles (gather kernel: elements), the workgroups launched, the tile kernel's LDS
            const bool tiled = e.variant == EW_TABLE_TILE;
            n = std::snprintf(buf, len, "{\"op\":\"elementwise\",\"variant\":%d,\"modes\":%u,\"tile\":[%u,%u,%u],\"kname\":\"%s\",\"blocks\":%u,\"grid\":%u,\"lds\":%u}",
                              e.variant, e.tab->nModes, e.tab->tilePos, e.tabFromA, e.tabFromD, tiled ? "ew_table_tile_kernel" : "ew_table_gather_kernel",
                              e.tab->total, e.tabGrid, tiled ? ew_table_lds_bytes((uint32_t)dtype_size(e.dtypeD)) : 0u);
            return describe_unary(buf, len, n, e.p.unA, 0, e.p.unC);
        }
        n = std::snprintf(buf, len, "{\"op\":\"elementwise\",\"variant\":%d,\"E0\":%u,\"E1\":%u,\"rest\":%u,\"blocks\":%u,\"tile0\":%u,\"order\":%u}",
                          e.variant, e.p.E0, e.p.E1, e.p.rest.total, e.p.nBlocks, e.p.tile0, e.p.order);
        n = describe_unary(buf, len, n, e.p.unA, 0, e.p.unC);
        // a converting plan (kernels/elementwise_convert.hip): the hipDataType values of A and of D
        if (e.converts() && n > 1 && (size_t)n < len && buf[n - 1] == '}')
            n = n - 1 + std::snprintf(buf + n - 1, len - (size_t)n + 1, ",\"convert\":[%d,%d]}", (int)e.dtypeA, (int)e.dtypeD);
        // a padded permutation: the elements the fill writes (the whole padded buffer) and the element offset of the interior, beside the inner plan's fields
        if (pl.kind == OpKind::Permutation && pl.padFillElems != 0 && n > 1 && (size_t)n < len && buf[n - 1] == '}')
            n = n - 1 + std::snprintf(buf + n - 1, len - (size_t)n + 1, ",\"pad\":[%llu,%lld]}", (unsigned long long)pl.padFillElems,
                                      (long long)pl.padOffsetElems);
    }
    return n;
}

}  // namespace ctamd

extern "C" {

// reduction.cu:219-222, einsum.cu:369-372
cutensorStatus_t cutensorReduce(const cutensorHandle_t handle, const cutensorPlan_t plan, const void* alpha,
                                const void* A, const void* beta, const void* C, void* D, void* workspace,
                                uint64_t workspaceSize, cudaStream_t stream) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || plan->kind != OpKind::Reduction) return CUTENSOR_STATUS_INVALID_VALUE;
    if (alpha == nullptr || beta == nullptr || A == nullptr || D == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    const CxScalar a = read_scalar(alpha, plan->scalarType), b = read_scalar(beta, plan->scalarType);   // complex data: complex scalars
    const bool betaSet = b.re != 0.0 || b.im != 0.0;
    if (betaSet && C == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (misaligned(A, plan->alignA) || misaligned(D, plan->alignD) || (betaSet && misaligned(C, plan->alignC)))
        return CUTENSOR_STATUS_INVALID_VALUE;
    hipError_t err;
    if (plan->red.isPermutation) {
        EwCall call;
        call.A = A; call.alpha = a; call.C = C; call.gamma = b; call.D = D;
        err = run_elementwise(plan->red.perm, plan->dtype, call, stream);
    } else if (plan->red.variant == RED_TABLE) {
        if (plan->requiredWorkspace > 0 && (workspace == nullptr || workspaceSize < plan->requiredWorkspace))
            return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
        if (!plan->red.tab) return CUTENSOR_STATUS_INTERNAL_ERROR;
        EwTable t = *plan->red.tab;
        t.A = A; t.C = betaSet ? C : nullptr; t.D = D;
        t.alpha64 = a.re; t.alphaIm = a.im; t.gamma64 = b.re; t.gammaIm = b.im;
        t.partial = (t.splitR > 1) ? workspace : nullptr;
        err = launch_reduce_table(t, (int)plan->dtype, plan->accumulate64 || plan->dtype == HIP_R_64F, stream);
    } else {
        if (plan->requiredWorkspace > 0 && (workspace == nullptr || workspaceSize < plan->requiredWorkspace))
            return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
        ReduceParams p = plan->red.p;
        p.A = A; p.C = betaSet ? C : D; p.D = D;
        p.alpha = (float)a.re; p.beta = (float)b.re; p.alpha64 = a.re; p.beta64 = b.re;
        p.alphaIm = a.im; p.betaIm = b.im;
        p.partial = (p.splitR > 1) ? workspace : nullptr;
        const bool acc64 = plan->accumulate64 || plan->dtype == HIP_R_64F;
        err = launch_reduce(p, plan->red.variant, (int)plan->dtype, acc64, stream);
        if (err == hipSuccess && p.splitR > 1) err = launch_reduce_finalize(p, (int)plan->dtype, acc64, stream);
    }
    if (err != hipSuccess) { CT_LOG("cutensorReduce: %s", hipGetErrorString(err)); return CUTENSOR_STATUS_EXECUTION_FAILED; }
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// elementwise_permute.cu:198-200
cutensorStatus_t cutensorPermute(const cutensorHandle_t handle, const cutensorPlan_t plan, const void* alpha,
                                 const void* A, void* B, const cudaStream_t stream) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || plan->kind != OpKind::Permutation) return CUTENSOR_STATUS_INVALID_VALUE;
    if (alpha == nullptr || A == nullptr || B == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (misaligned(A, plan->alignA) || misaligned(B, plan->alignD)) return CUTENSOR_STATUS_INVALID_VALUE;
    hipError_t err = hipSuccess;
    EwCall call;
    call.A = A; call.alpha = read_scalar(alpha, plan->scalarType); call.D = B;
    if (plan->padFillElems != 0) {   // border (and interior, rewritten next) = padding value
        // (border and offset in the OUTPUT's type: plan->dtype is A's, which a converting permutation tells apart)
        err = launch_fill(B, plan->padFillElems, (int)plan->ew.dtypeD, plan->padValue, stream);
        call.D = static_cast<char*>(B) + plan->padOffsetElems * (int64_t)dtype_size(plan->ew.dtypeD);
    }
    if (err == hipSuccess) err = run_elementwise(plan->ew, plan->dtype, call, stream);
    if (err != hipSuccess) { CT_LOG("cutensorPermute: %s", hipGetErrorString(err)); return CUTENSOR_STATUS_EXECUTION_FAILED; }
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// elementwise_binary.cu:202-205
cutensorStatus_t cutensorElementwiseBinaryExecute(const cutensorHandle_t handle, const cutensorPlan_t plan,
                                                  const void* alpha, const void* A, const void* gamma,
                                                  const void* C, void* D, cudaStream_t stream) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || plan->kind != OpKind::ElementwiseBinary) return CUTENSOR_STATUS_INVALID_VALUE;
    if (alpha == nullptr || gamma == nullptr || A == nullptr || C == nullptr || D == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (misaligned(A, plan->alignA) || misaligned(C, plan->alignC) || misaligned(D, plan->alignD)) return CUTENSOR_STATUS_INVALID_VALUE;
    EwCall call;
    call.A = A; call.alpha = read_scalar(alpha, plan->scalarType); call.C = C; call.gamma = read_scalar(gamma, plan->scalarType); call.D = D;
    const hipError_t err = run_elementwise(plan->ew, plan->dtype, call, stream);
    if (err != hipSuccess) { CT_LOG("cutensorElementwiseBinaryExecute: %s", hipGetErrorString(err)); return CUTENSOR_STATUS_EXECUTION_FAILED; }
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// elementwise_trinary.cu:223-227
cutensorStatus_t cutensorElementwiseTrinaryExecute(const cutensorHandle_t handle, const cutensorPlan_t plan,
                                                   const void* alpha, const void* A, const void* beta, const void* B,
                                                   const void* gamma, const void* C, void* D, cudaStream_t stream) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || plan->kind != OpKind::ElementwiseTrinary) return CUTENSOR_STATUS_INVALID_VALUE;
    if (alpha == nullptr || beta == nullptr || gamma == nullptr || A == nullptr || B == nullptr || C == nullptr || D == nullptr)
        return CUTENSOR_STATUS_INVALID_VALUE;
    if (misaligned(A, plan->alignA) || misaligned(B, plan->alignB3) || misaligned(C, plan->alignC) || misaligned(D, plan->alignD))
        return CUTENSOR_STATUS_INVALID_VALUE;
    const EwPasses run = trinary_passes(plan->ew3, A, B, C, D, read_scalar(alpha, plan->scalarType), read_scalar(beta, plan->scalarType),
                                        read_scalar(gamma, plan->scalarType));
    if (run.n == 0) return CUTENSOR_STATUS_NOT_SUPPORTED;
    hipError_t err = hipSuccess;
    for (int i = 0; i < run.n && err == hipSuccess; ++i) err = run_elementwise(*run.pass[i].ew, plan->dtype, run.pass[i].call, stream);
    if (err != hipSuccess) { CT_LOG("cutensorElementwiseTrinaryExecute: %s", hipGetErrorString(err)); return CUTENSOR_STATUS_EXECUTION_FAILED; }
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

}  // extern "C"
