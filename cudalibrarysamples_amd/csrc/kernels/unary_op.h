// unary_op.h — the per-operand unary operators of the element-wise and reduction families (elementwise.hip, reduce.hip):
// cutensorOperator_t SQRT / RELU / RCP / SIGMOID / TANH / EXP / LOG / ABS / NEG on real data.
//
// One device function, templated on the arithmetic type the running kernel already uses for the operand (float for fp32 / bf16 / fp16
// data, double for fp64 data and for fp32 data accumulated in 64 bits), selected by a wave-uniform operator code from the kernel's
// argument block (Ew2DParams::unA / unX / unE / unC, ReduceParams::unA / unC): a scalar branch, no divergence.  The operator is applied
// to the loaded element BEFORE its scalar; nothing is rounded to the data type between the operator and the final store.
//
// SQRT and RCP are the correctly rounded IEEE operations (the build has no fast-math flag: sqrt and the division compile to their
// correctly rounded expansions); EXP / LOG / TANH are the device library's functions, SIGMOID is 1 / (1 + exp(-x)) on top of it.
// Out-of-domain inputs follow IEEE: sqrt(-1) = NaN, 1 / 0 = +-inf, log(0) = -inf.
//
// Every kernel exists twice: the identity twin (UN = false) compiles none of this — un_apply<UN = false> returns its argument and the
// kernel is the code it was before the operators existed — and the operator twin (UN = true), which the launchers pick when an
// attached operand carries a code other than IDENTITY / CONJ (un_active).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ctamd {

enum {   // cutensorOperator_t values
    UN_IDENTITY = 1, UN_SQRT = 2, UN_RELU = 8, UN_CONJ = 9, UN_RCP = 10, UN_SIGMOID = 11, UN_TANH = 12,
    UN_EXP = 22, UN_LOG = 23, UN_ABS = 24, UN_NEG = 25
};

// true: the code names an operator that changes real data (0 = unset, IDENTITY and CONJ do not)
__host__ __device__ inline bool un_active(int32_t code) { return code != 0 && code != UN_IDENTITY && code != UN_CONJ; }

__device__ __forceinline__ float  un_sqrt(float x)  { return sqrtf(x); }
__device__ __forceinline__ double un_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float  un_exp(float x)   { return expf(x); }
__device__ __forceinline__ double un_exp(double x)  { return exp(x); }
__device__ __forceinline__ float  un_log(float x)   { return logf(x); }
__device__ __forceinline__ double un_log(double x)  { return log(x); }
__device__ __forceinline__ float  un_tanh(float x)  { return tanhf(x); }
__device__ __forceinline__ double un_tanh(double x) { return tanh(x); }
__device__ __forceinline__ float  un_abs(float x)   { return fabsf(x); }
__device__ __forceinline__ double un_abs(double x)  { return fabs(x); }

// N elements under ONE operator: the switch is outside the element loop
template <bool UN, typename S, int N>
__device__ __forceinline__ void un_apply_n(int32_t code, S (&v)[N]) {
    if constexpr (UN) {
        switch (code) {
#define CTAMD_UN_CASE(CODE, EXPR)                                     \
            case CODE:                                                \
                _Pragma("unroll") for (int i = 0; i < N; ++i) { const S x = v[i]; v[i] = (EXPR); } \
                break;
            CTAMD_UN_CASE(UN_SQRT, un_sqrt(x))
            CTAMD_UN_CASE(UN_RELU, x > (S)0 ? x : (S)0)
            CTAMD_UN_CASE(UN_RCP, (S)1 / x)
            CTAMD_UN_CASE(UN_SIGMOID, (S)1 / ((S)1 + un_exp(-x)))
            CTAMD_UN_CASE(UN_TANH, un_tanh(x))
            CTAMD_UN_CASE(UN_EXP, un_exp(x))
            CTAMD_UN_CASE(UN_LOG, un_log(x))
            CTAMD_UN_CASE(UN_ABS, un_abs(x))
            CTAMD_UN_CASE(UN_NEG, -x)
#undef CTAMD_UN_CASE
            default: break;      // IDENTITY, CONJ (a no-op on real data), 0
        }
    }
}

template <bool UN, typename S>
__device__ __forceinline__ S un_apply(int32_t code, S x) {
    S v[1] = {x};
    un_apply_n<UN, S, 1>(code, v);
    return v[0];
}

// the same on the accumulator type of an element-traits class (wide_elem.h); complex traits have no operator twin
template <class Tr, bool UN>
__device__ __forceinline__ typename Tr::Acc w_un(int32_t code, typename Tr::Acc x) {
    if constexpr (UN && !Tr::CX) return un_apply<true, typename Tr::Acc>(code, x);
    else return x;
}

typedef float un_f32x4 __attribute__((ext_vector_type(4)));
template <bool UN>
__device__ __forceinline__ un_f32x4 un_apply4(int32_t code, un_f32x4 x) {
    if constexpr (UN) {
        float v[4] = {x[0], x[1], x[2], x[3]};
        un_apply_n<true, float, 4>(code, v);
        return un_f32x4{v[0], v[1], v[2], v[3]};
    } else {
        return x;
    }
}

}  // namespace ctamd
