// elementwise_kernels.inc — the kernels of elementwise.hip that exist twice: elementwise.hip includes this file once with CTAMD_UN = false and
// CTAMD_KERNEL(x) = x_kernel (the identity twins: exactly the kernels that existed before the unary operators, un_apply<false> compiles to
// nothing) and once with CTAMD_UN = true and CTAMD_KERNEL(x) = x_un_kernel (the operator twins, unary_op.h).  No include guard on purpose.

// T0 = tile extent along dim0 (D's contiguous mode): 64, 128 or 256 floats = 256-B / 512-B / 1-KiB written row segments.
// The width of the WRITTEN segment is what moves the 2048^3 permutation (profiles/r03_transpose_sweep*.jsonl: 64 -> 6.14,
// 128 -> 6.45, 256 -> 6.56 TB/s with one workgroup per tile; the read width and the tile order do not matter), so the
// planner takes the widest T0 the extent fills (Ew2DParams::tile0).
// HASX: second permuted operand through a second LDS tile (a separate instantiation, so that the plain permutation
// keeps its smaller footprint)
// UN: the operator twin (unary_op.h) — the operators join in the write phase, on the values as they come out of LDS
template <bool HASX, int T0>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_transpose_f32)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    constexpr int LD = T0 + 4;                      // LDS row stride (floats)
    constexpr int RD_PASSES = T0 / 64;              // a read pass covers 64 dim0 rows (16 lane groups x 4 rows) x 64 dim1 floats
    constexpr int LPW = T0 / 4;                     // write: lanes per dim1 row
    constexpr int RPW = 256 / LPW;                  //        dim1 rows per pass
    constexpr int WR_PASSES = TT / RPW;
    __shared__ __attribute__((aligned(16))) float tile[TT * LD];   // [dim1][dim0]
    __shared__ __attribute__((aligned(16))) float tileX[HASX ? TT * LD : 4];
    const float* X = HASX ? static_cast<const float*>(p.X) : nullptr;
    const float* A = static_cast<const float*>(p.A);
    const float* C = static_cast<const float*>(p.C);
    const float* E = static_cast<const float*>(p.E);
    float*       D = static_cast<float*>(p.D);
    const int tid = threadIdx.x;

    const uint32_t nIds = p.order ? 8u * p.idsPerXcd : p.nBlocks;
    for (uint32_t b = blockIdx.x; b < nIds; b += gridDim.x) {
        TileId t;
        if (!ordered_tile(p, b, t)) continue;
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t i0 = t.t0 * T0, i1 = t.t1 * TT;   // tile origin (dim0, dim1)

        // interior tiles (all of them when the extents divide) take the unguarded path: every load of the tile is issued
        // before the first one is used, every store is a plain scaled copy
        const bool full = (i0 + T0 <= p.E0) && (i1 + TT <= p.E1);
        // ---- read: lane -> (dim1 float4 c1 = tid%16, dim0 block r0 = tid/16 [+ 64 per pass]), 4 dim0 rows each
        {
            const uint32_t c1 = i1 + 4 * (tid & 15);
            if (full) {
                const float* src = A + oA + (int64_t)(i0 + 4 * (tid >> 4)) * p.sA0 + c1;
                f32x4 in[RD_PASSES][4];
#pragma unroll
                for (int ps = 0; ps < RD_PASSES; ++ps)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        in[ps][r] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (int64_t)(64 * ps + r) * p.sA0));
#pragma unroll
                for (int ps = 0; ps < RD_PASSES; ++ps)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 o = {in[ps][0][j], in[ps][1][j], in[ps][2][j], in[ps][3][j]};
                        *reinterpret_cast<f32x4*>(&tile[(4 * (tid & 15) + j) * LD + 4 * (tid >> 4) + 64 * ps]) = o;
                    }
            } else {
                // edge tile: one pass at a time under per-row bounds tests.  (Round 6 tried the interior's two phases under predicates —
                // all loads of the tile first: 10 % SLOWER on 400 x 200 x 300, profiles/r06zc_*; what ragged extents cost is the row pitch,
                // 1200- and 1600-byte rows against 128-byte lines, not the rolled loop.)
#pragma unroll 1
                for (int ps = 0; ps < RD_PASSES; ++ps) {
                    const int      l0 = 4 * (tid >> 4) + 64 * ps;
                    const uint32_t r0 = i0 + l0;
                    f32x4 in[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        in[r] = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (c1 < p.E1 && (r0 + r) < p.E0)
                            in[r] = __builtin_nontemporal_load(
                                reinterpret_cast<const f32x4*>(A + oA + (int64_t)(r0 + r) * p.sA0 + c1));
                    }
                    // 4x4 register transpose: out[j] = (in[0][j], in[1][j], in[2][j], in[3][j])
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 o = {in[0][j], in[1][j], in[2][j], in[3][j]};
                        *reinterpret_cast<f32x4*>(&tile[(4 * (tid & 15) + j) * LD + l0]) = o;
                    }
                }
            }
            if constexpr (HASX) {
                const int64_t oX = rest_offset_x(p.rest, p.restX, t.rest);
                if (full) {      // as A's interior path: every load of the tile in flight before the first one is used (round 6)
                    const float* src = X + oX + (int64_t)(i0 + 4 * (tid >> 4)) * p.sX0 + c1;
                    f32x4 in[RD_PASSES][4];
#pragma unroll
                    for (int ps = 0; ps < RD_PASSES; ++ps)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            in[ps][r] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (int64_t)(64 * ps + r) * p.sX0));
#pragma unroll
                    for (int ps = 0; ps < RD_PASSES; ++ps)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const f32x4 o = {in[ps][0][j], in[ps][1][j], in[ps][2][j], in[ps][3][j]};
                            *reinterpret_cast<f32x4*>(&tileX[(4 * (tid & 15) + j) * LD + 4 * (tid >> 4) + 64 * ps]) = o;
                        }
                } else
#pragma unroll 1
                for (int ps = 0; ps < RD_PASSES; ++ps) {
                    const int      l0 = 4 * (tid >> 4) + 64 * ps;
                    const uint32_t r0 = i0 + l0;
                    f32x4 in[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        in[r] = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (c1 < p.E1 && (r0 + r) < p.E0)
                            in[r] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(X + oX + (int64_t)(r0 + r) * p.sX0 + c1));
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 o = {in[0][j], in[1][j], in[2][j], in[3][j]};
                        *reinterpret_cast<f32x4*>(&tileX[(4 * (tid & 15) + j) * LD + l0]) = o;
                    }
                }
            }
        }
        __syncthreads();
        // ---- write: lane -> (dim0 float4 c0 = tid % LPW, dim1 row = tid / LPW + RPW * pass)
        {
            const int      l0 = 4 * (tid % LPW);
            const uint32_t c0 = i0 + l0;
            if (!HASX && full && E == nullptr && C == nullptr) {
                float* dst = D + oD + (int64_t)(i1 + tid / LPW) * p.sD1 + c0;
#pragma unroll
                for (int pass = 0; pass < WR_PASSES; ++pass) {
                    f32x4 v = un_apply4<UN>(p.unA, *reinterpret_cast<const f32x4*>(&tile[(tid / LPW + RPW * pass) * LD + l0]));
                    v *= p.alpha;
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst + (int64_t)(RPW * pass) * p.sD1));
                }
            } else if (full && (C == nullptr || p.sC0 == 1)) {
                // interior tile of a binary / trinary form (round 6): the rows of C and E this lane combines with are requested for ALL
                // passes before the first one is used, no bounds tests — the rolled loop below serialises a load's latency per pass
                // (the sample's trinary form at 512 x 256 x 256: 4.4 TB/s against 5.4 for the plain permutation of the same tensor)
                const int64_t rowD = oD + (int64_t)(i1 + tid / LPW) * p.sD1 + c0;
                f32x4 cv[WR_PASSES], ev[WR_PASSES];
                if (C != nullptr) {
                    const float* cp = C + oC + (int64_t)(i1 + tid / LPW) * p.sC1 + c0;
#pragma unroll
                    for (int pass = 0; pass < WR_PASSES; ++pass)
                        cv[pass] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(cp + (int64_t)(RPW * pass) * p.sC1));
                }
                if (E != nullptr) {
#pragma unroll
                    for (int pass = 0; pass < WR_PASSES; ++pass)
                        ev[pass] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(E + rowD + (int64_t)(RPW * pass) * p.sD1));
                }
#pragma unroll
                for (int pass = 0; pass < WR_PASSES; ++pass) {
                    const int lr = tid / LPW + RPW * pass;
                    f32x4 v = un_apply4<UN>(p.unA, *reinterpret_cast<const f32x4*>(&tile[lr * LD + l0]));
                    v *= p.alpha;
                    if constexpr (HASX) v = ew_comb4(p.opAB, p.xi * un_apply4<UN>(p.unX, *reinterpret_cast<const f32x4*>(&tileX[lr * LD + l0])), v);
                    if (E != nullptr) v = ew_comb4(p.opAB, p.delta * un_apply4<UN>(p.unE, ev[pass]), v);
                    if (C != nullptr) v = ew_comb4(p.opAC, v, p.gamma * un_apply4<UN>(p.unC, cv[pass]));
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(D + rowD + (int64_t)(RPW * pass) * p.sD1));
                }
            } else {
#pragma unroll 1
                for (int pass = 0; pass < WR_PASSES; ++pass) {
                    const int      lr = tid / LPW + RPW * pass;
                    const uint32_t r1 = i1 + lr;
                    if (c0 < p.E0 && r1 < p.E1) {
                        f32x4 v = un_apply4<UN>(p.unA, *reinterpret_cast<const f32x4*>(&tile[lr * LD + l0]));
                        v *= p.alpha;
                        if constexpr (HASX)
                            v = ew_comb4(p.opAB, p.xi * un_apply4<UN>(p.unX, *reinterpret_cast<const f32x4*>(&tileX[lr * LD + l0])), v);
                        if (E != nullptr)
                            v = ew_comb4(p.opAB, p.delta * un_apply4<UN>(p.unE, *reinterpret_cast<const f32x4*>(E + oD + (int64_t)r1 * p.sD1 + c0)), v);
                        if (C != nullptr) {
                            const float* cp = C + oC + (int64_t)r1 * p.sC1 + (int64_t)c0 * p.sC0;
                            f32x4 c;
                            if (p.sC0 == 1) {
                                c = *reinterpret_cast<const f32x4*>(cp);
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e) c[e] = cp[(int64_t)e * p.sC0];
                            }
                            v = ew_comb4(p.opAC, v, p.gamma * un_apply4<UN>(p.unC, c));
                        }
                        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(D + oD + (int64_t)r1 * p.sD1 + c0));
                    }
                }
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_rowcopy_f32)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    const float* A = static_cast<const float*>(p.A);
    const float* C = static_cast<const float*>(p.C);
    const float* E = static_cast<const float*>(p.E);
    float*       D = static_cast<float*>(p.D);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * RC_T0 + 4 * (tid & 63);
        if (c0 >= p.E0) continue;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t r1 = t.t1 * RC_T1 + (tid >> 6) * 2 + r;
            if (r1 >= p.E1) continue;
            f32x4 v = un_apply4<UN>(p.unA, __builtin_nontemporal_load(
                reinterpret_cast<const f32x4*>(A + oA + (int64_t)r1 * p.sA1 + c0)));
            v *= p.alpha;
            if (E != nullptr)
                v = ew_comb4(p.opAB, p.delta * un_apply4<UN>(p.unE, *reinterpret_cast<const f32x4*>(E + oD + (int64_t)r1 * p.sD1 + c0)), v);
            if (C != nullptr) {
                const float* cp = C + oC + (int64_t)r1 * p.sC1 + (int64_t)c0 * p.sC0;
                f32x4 c;
                if (p.sC0 == 1) {
                    c = *reinterpret_cast<const f32x4*>(cp);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) c[e] = cp[(int64_t)e * p.sC0];
                }
                v = ew_comb4(p.opAC, v, p.gamma * un_apply4<UN>(p.unC, c));
            }
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(D + oD + (int64_t)r1 * p.sD1 + c0));
        }
    }
}

template <bool BF>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_rowcopy_h16)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    const uint16_t* A = static_cast<const uint16_t*>(p.A);
    const uint16_t* C = static_cast<const uint16_t*>(p.C);
    const uint16_t* E = static_cast<const uint16_t*>(p.E);
    uint16_t*       D = static_cast<uint16_t*>(p.D);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * 512 + 8 * (tid & 63);
        if (c0 >= p.E0) continue;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t r1 = t.t1 * 8 + (tid >> 6) * 2 + r;
            if (r1 >= p.E1) continue;
            float a[8];
            h16_unpack<BF>(__builtin_nontemporal_load(reinterpret_cast<const u32x4e*>(A + oA + (int64_t)r1 * p.sA1 + c0)), a);
            const int64_t offD = oD + (int64_t)r1 * p.sD1 + c0;
            const u32x4e out = h16_combine<BF, UN>(p, a, E, C, offD, oC + (int64_t)r1 * p.sC1 + (int64_t)c0 * p.sC0);
            __builtin_nontemporal_store(out, reinterpret_cast<u32x4e*>(D + offD));
        }
    }
}

template <bool BF>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_transpose_h16)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    constexpr int PITCH = 65;
    __shared__ uint16_t tile[64 * PITCH];   // [dim1][dim0]
    const uint16_t* A = static_cast<const uint16_t*>(p.A);
    const uint16_t* C = static_cast<const uint16_t*>(p.C);
    const uint16_t* E = static_cast<const uint16_t*>(p.E);
    uint16_t*       D = static_cast<uint16_t*>(p.D);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t i0 = t.t0 * 64, i1 = t.t1 * 64;
        // read: unit u = 8 dim1 elements of one dim0 row (8 lanes cover a 128-byte segment)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int u = tid + 256 * k;
            const uint32_t r0 = u >> 3, c1 = 8 * (u & 7);
            u32x4e v = {0u, 0u, 0u, 0u};
            if (i0 + r0 < p.E0 && i1 + c1 < p.E1)
                v = __builtin_nontemporal_load(reinterpret_cast<const u32x4e*>(A + oA + (int64_t)(i0 + r0) * p.sA0 + i1 + c1));
#pragma unroll
            for (int j = 0; j < 8; ++j) tile[(c1 + j) * PITCH + r0] = (uint16_t)(v[j >> 1] >> (16 * (j & 1)));
        }
        __syncthreads();
        // write: unit u = 8 dim0 elements of one dim1 row
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int u = tid + 256 * k;
            const uint32_t lr = u >> 3, c0 = 8 * (u & 7);
            if (i0 + c0 < p.E0 && i1 + lr < p.E1) {
                float a[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = h16_to_f32<BF>(tile[lr * PITCH + c0 + j]);
                const int64_t offD = oD + (int64_t)(i1 + lr) * p.sD1 + i0 + c0;
                const u32x4e out = h16_combine<BF, UN>(p, a, E, C, offD, oC + (int64_t)(i1 + lr) * p.sC1 + (int64_t)(i0 + c0) * p.sC0);
                __builtin_nontemporal_store(out, reinterpret_cast<u32x4e*>(D + offD));
            }
        }
        __syncthreads();
    }
}

// 16-bit transposing kernel for FULL tiles of T0 (dim0: 128 / 256 elements = 256-B / 512-B written row segments) x 64 (dim1:
// 128-B read segments); the planner selects it when the extents divide (no edge guards), the 64 x 64 kernel above otherwise.
// A lane loads one 8 x 8 block (8 dim0 rows x 16 bytes along dim1), transposes it in registers with byte permutes and parks it
// as eight 16-byte pieces of the [dim1][dim0] LDS image; the write pass reads 16-byte pieces along dim0.  alpha == 1 without
// E / C terms and without a unary operator is a bit copy.  Same lessons as the fp32 kernel: the WRITTEN segment width is what counts, one workgroup per tile.
template <bool BF, int T0, int T1>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_transpose_h16_wide)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    constexpr int PITCH = T0 + 8;                   // elements; rows stay 16-byte aligned
    constexpr int OCT = T1 / 8;                     // read: 16-byte octets per dim0 row
    constexpr int BROWS = 256 / OCT;                //       8-row blocks per pass
    constexpr int RP = 8 * BROWS;                   //       dim0 rows per pass
    constexpr int RD_PASSES = (T0 + RP - 1) / RP;
    constexpr int RD_LANES = (T0 >= RP) ? 256 : (T0 / 8) * OCT;   // a 128 x 64 tile keeps half the lanes busy while reading
    constexpr int LPW = T0 / 8;                     // write: lanes per dim1 row
    constexpr int RPW = 256 / LPW;
    constexpr int WR_PASSES = T1 / RPW;
    static_assert((T0 == 256 || T0 == 128) && (T1 == 64 || T1 == 128), "tiles built: {128, 256} x {64, 128}");
    __shared__ __attribute__((aligned(16))) uint16_t tile[T1 * PITCH];   // [dim1][dim0]
    const uint16_t* A = static_cast<const uint16_t*>(p.A);
    const uint16_t* C = static_cast<const uint16_t*>(p.C);
    const uint16_t* E = static_cast<const uint16_t*>(p.E);
    uint16_t*       D = static_cast<uint16_t*>(p.D);
    const int tid = threadIdx.x;
    const uint32_t nIds = p.order ? 8u * p.idsPerXcd : p.nBlocks;
    for (uint32_t b = blockIdx.x; b < nIds; b += gridDim.x) {
        TileId t;
        if (!ordered_tile(p, b, t)) continue;
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t i0 = t.t0 * T0, i1 = t.t1 * T1;
        // ---- read + 8 x 8 register transpose
        if (tid < RD_LANES) {
            const int oct = tid % OCT;                                    // dim1 octet
            const int brow = tid / OCT;                                   // block row inside a pass
#pragma unroll
            for (int ps = 0; ps < RD_PASSES; ++ps) {
                const int r0 = 8 * brow + RP * ps;                        // first dim0 row of the block
                const uint16_t* src = A + oA + (int64_t)(i0 + r0) * p.sA0 + i1 + 8 * oct;
                u32x4e v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4e*>(src + (int64_t)k * p.sA0));
                // out[j] = (v[0].e[j], ..., v[7].e[j]); element j of v[k] is half (j & 1) of word j >> 1
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    u32x4e o;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const uint32_t lo = v[2 * w][j >> 1], hi = v[2 * w + 1][j >> 1];
                        o[w] = (j & 1) ? __builtin_amdgcn_perm(hi, lo, 0x07060302u) : __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                    }
                    *reinterpret_cast<u32x4e*>(&tile[(8 * oct + j) * PITCH + r0]) = o;
                }
            }
        }
        __syncthreads();
        // ---- write: 16-byte pieces along dim0
        {
            const int l0 = 8 * (tid % LPW);
            const bool plain = !UN && (E == nullptr && C == nullptr && p.alpha == 1.0f);
            uint16_t* dst = D + oD + (int64_t)(i1 + tid / LPW) * p.sD1 + i0 + l0;
#pragma unroll
            for (int pass = 0; pass < WR_PASSES; ++pass) {
                const int lr = tid / LPW + RPW * pass;
                u32x4e v = *reinterpret_cast<const u32x4e*>(&tile[lr * PITCH + l0]);
                if (!plain) {
                    float a[8];
                    h16_unpack<BF>(v, a);
                    const int64_t offD = oD + (int64_t)(i1 + lr) * p.sD1 + i0 + l0;
                    v = h16_combine<BF, UN>(p, a, E, C, offD, oC + (int64_t)(i1 + lr) * p.sC1 + (int64_t)(i0 + l0) * p.sC0);
                }
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4e*>(dst + (int64_t)(RPW * pass) * p.sD1));
            }
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_generic)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    typedef typename EwScalar<T>::type S;
    const T* A = static_cast<const T*>(p.A);
    const T* C = static_cast<const T*>(p.C);
    const T* E = static_cast<const T*>(p.E);
    T*       D = static_cast<T*>(p.D);
    const S alpha = sizeof(S) == 8 ? (S)p.alpha64 : (S)p.alpha;
    const S gamma = sizeof(S) == 8 ? (S)p.gamma64 : (S)p.gamma;
    const S delta = sizeof(S) == 8 ? (S)p.delta64 : (S)p.delta;
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * GN_T0 + (tid & 63);
        const uint32_t r1 = t.t1 * GN_T1 + (tid >> 6);
        if (c0 >= p.E0 || r1 >= p.E1) continue;
        S v = alpha * un_apply<UN, S>(p.unA, ew_load<T>(A + oA + (int64_t)c0 * p.sA0 + (int64_t)r1 * p.sA1));
        if (E != nullptr) v = ew_comb<S>(p.opAB, delta * un_apply<UN, S>(p.unE, ew_load<T>(E + oD + (int64_t)c0 * p.sD0 + (int64_t)r1 * p.sD1)), v);
        if (p.X != nullptr) {
            const S xi = sizeof(S) == 8 ? (S)p.xi64 : (S)p.xi;
            v = ew_comb<S>(p.opAB, xi * un_apply<UN, S>(p.unX, ew_load<T>(static_cast<const T*>(p.X) + rest_offset_x(p.rest, p.restX, t.rest) +
                                                                          (int64_t)c0 * p.sX0 + (int64_t)r1 * p.sX1)), v);
        }
        if (C != nullptr) v = ew_comb<S>(p.opAC, v, gamma * un_apply<UN, S>(p.unC, ew_load<T>(C + oC + (int64_t)c0 * p.sC0 + (int64_t)r1 * p.sC1)));
        ew_store<T>(D + oD + (int64_t)c0 * p.sD0 + (int64_t)r1 * p.sD1, v);
    }
}

// ---------------------------------------------------------------------------------------------
// EW_TRANSPOSE_ANY (round 6): D = alpha * perm(A) with D contiguous along dim0 and A along dim1 — the transposing kernels' case — at ANY
// extents, strides and base alignment (odd extents, 2-byte-aligned pointers: what the 16-byte-lane kernels refuse and the element-gather
// kernel above runs at 0.9-1.5 TB/s, each lane of a load on another 64-byte line).  A 64 x 64 tile through LDS, element by element:
// loads walk dim1 (A's contiguous mode), stores walk dim0 (D's), both coalesced; the LDS row pitch of 65 (fp32) / 66 (16-bit) elements
// keeps the column reads off a single bank.  HBM-bound: 2 |D| bytes.
// ---------------------------------------------------------------------------------------------
// HASC: the binary form D = opAC(alpha perm(A), gamma C) (elementwise_binary.cu:149-153) — C joins in the store phase, along D's contiguous
// mode; an instantiation of its own, so that the plain permutation carries no operand test in its store loop.
template <typename T, bool HASC>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_transpose_any)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    constexpr int PITCH = sizeof(T) == 4 ? 65 : 66;
    __shared__ T lds[64 * PITCH];
    const T* A = static_cast<const T*>(p.A);
    const T* C = static_cast<const T*>(p.C);
    T*       D = static_cast<T*>(p.D);
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    const bool raw = !UN && p.alpha == 1.0f;           // (a unary operator leaves the bit copy)
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * 64u, r0 = t.t1 * 64u;            // tile origin along dim0 / dim1
        const uint32_t n0 = (p.E0 - c0 < 64u) ? (p.E0 - c0) : 64u, n1 = (p.E1 - r0 < 64u) ? (p.E1 - r0) : 64u;
        // in: lane = position along dim1 (A's stride-1 mode), four dim0 positions per pass
        if ((uint32_t)lane < n1) {
            const T* src = A + oA + (int64_t)(r0 + (uint32_t)lane) + (int64_t)c0 * p.sA0;
#pragma unroll 4
            for (uint32_t i = (uint32_t)row; i < n0; i += 4u) lds[i * PITCH + lane] = src[(int64_t)i * p.sA0];
        }
        __syncthreads();
        // out: lane = position along dim0 (D's stride-1 mode), four dim1 positions per pass
        if ((uint32_t)lane < n0) {
            T* dst = D + oD + (int64_t)(c0 + (uint32_t)lane) + (int64_t)r0 * p.sD1;
            if constexpr (HASC) {
                const T* csrc = C + oC + (int64_t)(c0 + (uint32_t)lane) * p.sC0 + (int64_t)r0 * p.sC1;
#pragma unroll 4
                for (uint32_t j = (uint32_t)row; j < n1; j += 4u) {
                    const T v = lds[lane * PITCH + j];
                    ew_store<T>(dst + (int64_t)j * p.sD1, ew_comb<float>(p.opAC, p.alpha * un_apply<UN, float>(p.unA, ew_load<T>(&v)),
                                                                        p.gamma * un_apply<UN, float>(p.unC, ew_load<T>(csrc + (int64_t)j * p.sC1))));
                }
            } else {
#pragma unroll 4
                for (uint32_t j = (uint32_t)row; j < n1; j += 4u) {
                    const T v = lds[lane * PITCH + j];
                    if (raw) dst[(int64_t)j * p.sD1] = v;
                    else ew_store<T>(dst + (int64_t)j * p.sD1, p.alpha * un_apply<UN, float>(p.unA, ew_load<T>(&v)));
                }
            }
        }
        __syncthreads();
    }
}

// The same for 16-bit elements in PAIRS (Ew2DParams::tile0 == 128): even extents and strides, 4-byte-aligned bases — a lane loads two
// neighbouring elements along A's contiguous mode (one 4-byte load) and stores two along D's, a 128 x 128 tile through LDS (row pitch 130):
// the element-by-element form moves 128 bytes per wave instruction and stops at 3.3 TB/s on bf16.  Pure permutations (alpha as above).
template <typename T>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_transpose_any_pair)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    constexpr int PITCH = 130;
    __shared__ __attribute__((aligned(4))) T lds[128 * PITCH];
    const T* A = static_cast<const T*>(p.A);
    T*       D = static_cast<T*>(p.D);
    const uint32_t lane = threadIdx.x & 63u, row = threadIdx.x >> 6;
    const bool raw = !UN && p.alpha == 1.0f;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * 128u, r0 = t.t1 * 128u;
        const uint32_t n0 = (p.E0 - c0 < 128u) ? (p.E0 - c0) : 128u, n1 = (p.E1 - r0 < 128u) ? (p.E1 - r0) : 128u;   // (even)
        if (2u * lane < n1) {
            const T* src = A + oA + (int64_t)(r0 + 2u * lane) + (int64_t)c0 * p.sA0;
#pragma unroll 4
            for (uint32_t i = row; i < n0; i += 4u)
                *reinterpret_cast<uint32_t*>(&lds[i * PITCH + 2u * lane]) = *reinterpret_cast<const uint32_t*>(src + (int64_t)i * p.sA0);
        }
        __syncthreads();
        if (2u * lane < n0) {
            T* dst = D + oD + (int64_t)(c0 + 2u * lane) + (int64_t)r0 * p.sD1;
#pragma unroll 4
            for (uint32_t j = row; j < n1; j += 4u) {
                T v0 = lds[(2u * lane) * PITCH + j], v1 = lds[(2u * lane + 1u) * PITCH + j];
                if (!raw) {
                    T w0, w1;
                    ew_store<T>(&w0, p.alpha * un_apply<UN, float>(p.unA, ew_load<T>(&v0)));
                    ew_store<T>(&w1, p.alpha * un_apply<UN, float>(p.unA, ew_load<T>(&v1)));
                    v0 = w0; v1 = w1;
                }
                uint16_t b0, b1;
                __builtin_memcpy(&b0, &v0, 2);
                __builtin_memcpy(&b1, &v1, 2);
                *reinterpret_cast<uint32_t*>(dst + (int64_t)j * p.sD1) = (uint32_t)b0 | ((uint32_t)b1 << 16);
            }
        }
        __syncthreads();
    }
}

template <class Tr, int T0, int T1>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_transpose_wide)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    constexpr int NV = Tr::NV;
    constexpr int LD = T0 + NV;                     // LDS row stride (elements)
    constexpr int LPR = T1 / NV;                    // read: lanes per dim0 row
    constexpr int RPP = (256 / LPR) * NV;           //       dim0 rows per pass
    constexpr int RD_PASSES = T0 / RPP;
    constexpr int LPW = T0 / NV;                    // write: lanes per dim1 row
    constexpr int RPW = 256 / LPW;                  //        dim1 rows per pass
    constexpr int WR_PASSES = T1 / RPW;
    static_assert(T0 % RPP == 0 && T1 % RPW == 0 && 256 % LPR == 0 && 256 % LPW == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) Elem tile[T1 * LD];   // [dim1][dim0]
    const Elem* A = static_cast<const Elem*>(p.A);
    const Elem* C = static_cast<const Elem*>(p.C);
    Elem*       D = static_cast<Elem*>(p.D);
    const int tid = threadIdx.x;
    const bool conjA = Tr::CX && p.conjA != 0;
    const uint32_t nIds = p.order ? 8u * p.idsPerXcd : p.nBlocks;
    for (uint32_t b = blockIdx.x; b < nIds; b += gridDim.x) {
        TileId t;
        if (!ordered_tile(p, b, t)) continue;
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t i0 = t.t0 * T0, i1 = t.t1 * T1;
        const bool full = (i0 + T0 <= p.E0) && (i1 + T1 <= p.E1);
        {   // ---- read: lane -> (dim1 unit c1 = tid % LPR, dim0 rows r0 .. r0 + NV - 1), RD_PASSES passes
            const int      l1 = NV * (tid % LPR);
            const uint32_t c1 = i1 + l1;
            wu32x4 in[RD_PASSES][NV];
#pragma unroll
            for (int ps = 0; ps < RD_PASSES; ++ps) {
                const uint32_t r0 = i0 + NV * (tid / LPR) + RPP * ps;
#pragma unroll
                for (int r = 0; r < NV; ++r) {
                    in[ps][r] = wu32x4{0u, 0u, 0u, 0u};
                    if (full || (c1 < p.E1 && (r0 + r) < p.E0))
                        in[ps][r] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(A + oA + (int64_t)(r0 + r) * p.sA0 + c1));
                }
            }
#pragma unroll
            for (int ps = 0; ps < RD_PASSES; ++ps) {
                const int l0 = NV * (tid / LPR) + RPP * ps;
                // NV x NV register transpose: unit j of the output = element j of every input row
                Acc v[NV][NV];
#pragma unroll
                for (int r = 0; r < NV; ++r) Tr::unpack(in[ps][r], v[r], conjA);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    Acc o[NV];
#pragma unroll
                    for (int r = 0; r < NV; ++r) o[r] = v[r][j];
                    *reinterpret_cast<wu32x4*>(&tile[(l1 + j) * LD + l0]) = Tr::pack(o);
                }
            }
        }
        __syncthreads();
        {   // ---- write: lane -> (dim0 unit c0 = tid % LPW, dim1 row tid / LPW + RPW * pass)
            const int      l0 = NV * (tid % LPW);
            const uint32_t c0 = i0 + l0;
#pragma unroll 2
            for (int pass = 0; pass < WR_PASSES; ++pass) {
                const int      lr = tid / LPW + RPW * pass;
                const uint32_t r1 = i1 + lr;
                if (full || (c0 < p.E0 && r1 < p.E1)) {
                    Acc v[NV];
                    Tr::unpack(*reinterpret_cast<const wu32x4*>(&tile[lr * LD + l0]), v, false);
#pragma unroll
                    for (int e = 0; e < NV; ++e)
                        v[e] = w_ew_finish<Tr, UN>(p, v[e], C + oC + (int64_t)r1 * p.sC1 + (int64_t)(c0 + e) * p.sC0, C != nullptr);
                    __builtin_nontemporal_store(Tr::pack(v), reinterpret_cast<wu32x4*>(D + oD + (int64_t)r1 * p.sD1 + c0));
                }
            }
        }
        __syncthreads();
    }
}

// row copy: A and D share the stride-1 mode — tile = 64 lanes x NV dim0 elements x 8 dim1 rows (4 waves x 2 rows), no LDS
template <class Tr>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(ew_rowcopy_wide)(const Ew2DParams p) {
    constexpr bool UN = CTAMD_UN;
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    constexpr int NV = Tr::NV;
    const Elem* A = static_cast<const Elem*>(p.A);
    const Elem* C = static_cast<const Elem*>(p.C);
    Elem*       D = static_cast<Elem*>(p.D);
    const int tid = threadIdx.x;
    const bool conjA = Tr::CX && p.conjA != 0;
    for (uint32_t b = blockIdx.x; b < p.nBlocks; b += gridDim.x) {
        const TileId t = decode_tile(p, b);
        int64_t oA, oD, oC;
        rest_offsets(p.rest, t.rest, oA, oD, oC);
        const uint32_t c0 = t.t0 * (64u * NV) + (uint32_t)NV * (tid & 63);
        if (c0 >= p.E0) continue;
        wu32x4 raw[2];
        uint32_t r1[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            r1[r] = t.t1 * 8u + (tid >> 6) * 2 + r;
            raw[r] = wu32x4{0u, 0u, 0u, 0u};
            if (r1[r] < p.E1) raw[r] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(A + oA + (int64_t)r1[r] * p.sA1 + c0));
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r1[r] >= p.E1) continue;
            Acc v[NV];
            Tr::unpack(raw[r], v, conjA);
#pragma unroll
            for (int e = 0; e < NV; ++e)
                v[e] = w_ew_finish<Tr, UN>(p, v[e], C + oC + (int64_t)r1[r] * p.sC1 + (int64_t)(c0 + e) * p.sC0, C != nullptr);
            __builtin_nontemporal_store(Tr::pack(v), reinterpret_cast<wu32x4*>(D + oD + (int64_t)r1[r] * p.sD1 + c0));
        }
    }
}
