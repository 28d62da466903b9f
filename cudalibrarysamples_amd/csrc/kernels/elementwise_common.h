// elementwise_common.h — device helpers shared by the element-wise translation units (elementwise.hip, elementwise_convert.hip and
// elementwise_trinary_cplx.hip):
// the fast division, the offsets of a rest index, the tile decomposition with its two tile orders, the binary combiners and the
// conversions between 16-bit storage and fp32.  Moved here unchanged from elementwise.hip when the converting kernels arrived.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "params.h"

namespace ctamd {

__device__ __forceinline__ uint32_t ew_fast_div(uint32_t n, const FastDiv& d) {
    return (d.d < 2) ? n : (__umulhi(n, d.magic) >> d.shift);
}

// offsets of a rest index in A (slot 0), D (slot 1) and C (slot 2)
__device__ __forceinline__ void rest_offsets(const ModeGroup& g, uint32_t idx, int64_t& oA, int64_t& oD,
                                             int64_t& oC) {
    oA = oD = oC = 0;
#pragma unroll
    for (int i = 0; i < kMaxGroupModes; ++i) {   // padding modes: {d = 1, magic = 0, stride = 0}
        const uint32_t q = __umulhi(idx, g.div[i].magic) >> g.div[i].shift;
        const uint32_t digit = idx - q * g.div[i].d;
        oA += (int64_t)digit * g.stride[0][i];
        oD += (int64_t)digit * g.stride[1][i];
        oC += (int64_t)digit * g.stride[2][i];
        idx = q;
    }
}

// offset of a rest index in the second permuted operand X (explicit stride array, same digits as rest_offsets)
__device__ __forceinline__ int64_t rest_offset_x(const ModeGroup& g, const int64_t* sx, uint32_t idx) {
    int64_t o = 0;
#pragma unroll
    for (int i = 0; i < kMaxGroupModes; ++i) {
        const uint32_t q = __umulhi(idx, g.div[i].magic) >> g.div[i].shift;
        o += (int64_t)(idx - q * g.div[i].d) * sx[i];
        idx = q;
    }
    return o;
}

// binary combiners of the element-wise family (cutensorOperator_t values; 0 = ADD)
template <typename S>
__device__ __forceinline__ S ew_comb(int op, S x, S y) {
    switch (op) {
        case 5: return x * y;                 // CUTENSOR_OP_MUL
        case 6: return x > y ? x : y;         // CUTENSOR_OP_MAX
        case 7: return x < y ? x : y;         // CUTENSOR_OP_MIN
        default: return x + y;                // CUTENSOR_OP_ADD
    }
}

struct TileId { uint32_t t0, t1, rest; };
__device__ __forceinline__ TileId decode_tile(const Ew2DParams& p, uint32_t b) {
    TileId t;
    uint32_t q = ew_fast_div(b, p.divTiles0);
    t.t0 = b - q * p.tiles0;
    const uint32_t q2 = ew_fast_div(q, p.divTiles1);
    t.t1 = q - q2 * p.tiles1;
    t.rest = q2;
    return t;
}

// Tile of workgroup-loop index b under the planner's tile order (Ew2DParams::order); false = this index names no tile.
//   order 0: ids walk dim0 tiles, dim1 tiles, rest.
//   order 1 (both the rows A is read by and the rows D is written by lie a large pitch apart, e.g. the full reversal
//   A[a,b,c] -> C[c,b,a] at 2048^3, 16 MiB on both sides): ids walk rest, then dim1, then dim0, and XCD x = workgroup id % 8
//   takes the x-th eighth of that sequence, so that at any time one XCD works inside a few dim0 / dim1 tiles — a few hundred
//   distinct pages per XCD instead of every page of both tensors (fp32: 5.79 -> 6.31 TB/s, profiles/r03_transpose_sweep3_rev.jsonl;
//   the same order WITHOUT the per-XCD split is the worst: 4.14)
__device__ __forceinline__ bool ordered_tile(const Ew2DParams& p, uint32_t b, TileId& t) {
    if (p.order == 0) { t = decode_tile(p, b); return true; }
    const uint32_t id = (b & 7u) * p.idsPerXcd + (b >> 3);
    if (id >= p.nBlocks) return false;
    const uint32_t q = ew_fast_div(id, p.divRest);
    t.rest = id - q * p.rest.total;
    const uint32_t q2 = ew_fast_div(q, p.divTiles1);
    t.t1 = q - q2 * p.tiles1;
    t.t0 = q2;
    return true;
}

typedef uint32_t u32x4e __attribute__((ext_vector_type(4)));

template <bool BF> __device__ __forceinline__ float h16_to_f32(uint16_t v) {
    if constexpr (BF) return __uint_as_float((uint32_t)v << 16);
    else return (float)__builtin_bit_cast(_Float16, v);
}
template <bool BF> __device__ __forceinline__ uint16_t f32_to_h16(float f) {
    if constexpr (BF) {
        uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    } else {
        return __builtin_bit_cast(uint16_t, (_Float16)f);
    }
}

}  // namespace ctamd
