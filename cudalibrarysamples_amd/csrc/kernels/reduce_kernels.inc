// reduce_kernels.inc — the kernels of reduce.hip that exist twice: reduce.hip includes this file once with CTAMD_UN = false and
// CTAMD_KERNEL(x) = x_kernel (the identity twins: exactly the kernels that existed before the unary operators, un_apply<false> compiles to
// nothing) and once with CTAMD_UN = true and CTAMD_KERNEL(x) = x_un_kernel (the operator twins, unary_op.h).  No include guard on purpose.

// ---------------------------------------------------------------------------------------------
// RED_COL, fp32.  grid.x covers kept float4 units, grid.y = splitR.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) CTAMD_KERNEL(reduce_col_f32)(const ReduceParams p) {
    constexpr bool UN = CTAMD_UN;
    const uint32_t unit = blockIdx.x * 256u + threadIdx.x;
    const uint32_t kv = unit * 4u;
    if (kv >= p.kept.total) return;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * p.redPerSplit;
    uint32_t rEnd = rBegin + p.redPerSplit;
    if (rEnd > p.red.total) rEnd = p.red.total;
    const int op = p.op;
    const float* A = static_cast<const float*>(p.A) + rd_offset<0>(p.kept, kv);
    f32x4 acc;
    for (int e = 0; e < 4; ++e) acc[e] = red_identity<float>(op);
    uint32_t r = rBegin;
    // eight rows (8 x 16 B per lane) in flight per iteration while the reduced index walks ONE mode with a constant stride (the
    // common case: no per-row offset arithmetic between the loads); four rows otherwise
    if (p.red.n == 1) {
        const int64_t step = p.red.stride[0][0];
        const float* q = A + (int64_t)r * step;
        for (; r + 8 <= rEnd; r += 8, q += 8 * step) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q + (int64_t)u * step));
            if constexpr (UN) {
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = un_apply4<true>(p.unA, v[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = red_apply<float>(op, acc[e], v[u][e]);
        }
    }
    for (; r + 4 <= rEnd; r += 4) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(A + rd_offset<0>(p.red, r + u)));
        if constexpr (UN) {
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = un_apply4<true>(p.unA, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = red_apply<float>(op, acc[e], v[u][e]);
    }
    for (; r < rEnd; ++r) {
        const f32x4 v = un_apply4<UN>(p.unA, *reinterpret_cast<const f32x4*>(A + rd_offset<0>(p.red, r)));
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = red_apply<float>(op, acc[e], v[e]);
    }
    if (p.partial != nullptr) {
        float* P = static_cast<float*>(p.partial) + (size_t)split * p.kept.total + kv;
        *reinterpret_cast<f32x4*>(P) = acc;
        return;
    }
    float*       D = static_cast<float*>(p.D);
    const float* C = static_cast<const float*>(p.C);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // kept mode 0 is contiguous in A; in D / C it may have any stride
        const int64_t oD = rd_offset<1>(p.kept, kv + e);
        float val = p.alpha * acc[e];
        if (p.beta != 0.f) val += p.beta * un_apply<UN, float>(p.unC, C[rd_offset<2>(p.kept, kv + e)]);
        D[oD] = val;
    }
}

// ---------------------------------------------------------------------------------------------
// RED_ROW, fp32.  One wave per (kept element, split); grid.x covers kept/4 (4 waves per block),
// grid.y = splitR.  redPerSplit is a multiple of 4 and red mode 0 is contiguous with extent % 4 == 0.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) CTAMD_KERNEL(reduce_row_f32)(const ReduceParams p) {
    constexpr bool UN = CTAMD_UN;
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (k >= p.kept.total) return;
    const int lane = threadIdx.x & 63;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * p.redPerSplit;
    uint32_t rEnd = rBegin + p.redPerSplit;
    if (rEnd > p.red.total) rEnd = p.red.total;
    const int op = p.op;
    const float* A = static_cast<const float*>(p.A) + rd_offset<0>(p.kept, k);
    float acc = red_identity<float>(op);
    uint32_t r = rBegin + 4u * lane;
    for (; r + 3u * 256u < rEnd; r += 4u * 256u) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(A + rd_offset<0>(p.red, r + 256u * u)));
        if constexpr (UN) {
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = un_apply4<true>(p.unA, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = red_apply<float>(op, acc, v[u][e]);
    }
    for (; r < rEnd; r += 256u) {
        f32x4 v = *reinterpret_cast<const f32x4*>(A + rd_offset<0>(p.red, r));
        if constexpr (UN) v = un_apply4<true>(p.unA, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = red_apply<float>(op, acc, v[e]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = red_apply<float>(op, acc, __shfl_down(acc, off, 64));
    if (lane != 0) return;
    if (p.partial != nullptr) {
        static_cast<float*>(p.partial)[(size_t)split * p.kept.total + k] = acc;
        return;
    }
    float val = p.alpha * acc;
    if constexpr (UN) {
        if (p.beta != 0.f) val += p.beta * un_apply<true, float>(p.unC, static_cast<const float*>(p.C)[rd_offset<2>(p.kept, k)]);
    } else {
        if (p.beta != 0.f) val += p.beta * static_cast<const float*>(p.C)[rd_offset<2>(p.kept, k)];
    }
    static_cast<float*>(p.D)[rd_offset<1>(p.kept, k)] = val;
}

template <class Tr>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(reduce_col_wide)(const ReduceParams p) {
    constexpr bool UN = CTAMD_UN;
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    constexpr int NV = Tr::NV;
    const uint32_t unit = blockIdx.x * 256u + threadIdx.x;
    const uint32_t kv = unit * (uint32_t)NV;
    if (kv >= p.kept.total) return;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * p.redPerSplit;
    uint32_t rEnd = rBegin + p.redPerSplit;
    if (rEnd > p.red.total) rEnd = p.red.total;
    const int op = p.op;
    const bool conj = Tr::CX && p.conjA != 0;
    const Elem* A = static_cast<const Elem*>(p.A) + rd_offset<0>(p.kept, kv);
    Acc acc[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] = Tr::identity(op);
    uint32_t r = rBegin;
    if (p.red.n == 1) {        // one reduced mode: eight rows in flight per lane, addresses one addition apart
        const int64_t step = p.red.stride[0][0];
        const Elem* q = A + (int64_t)r * step;
        for (; r + 8 <= rEnd; r += 8, q += 8 * step) {
            wu32x4 raw[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) raw[u] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(q + (int64_t)u * step));
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                Acc v[NV];
                Tr::unpack(raw[u], v, conj);
                if constexpr (UN && !Tr::CX) un_apply_n<true, Acc, NV>(p.unA, v);
#pragma unroll
                for (int e = 0; e < NV; ++e) acc[e] = Tr::apply(op, acc[e], v[e]);
            }
        }
    }
    for (; r + 4 <= rEnd; r += 4) {
        wu32x4 raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) raw[u] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(A + rd_offset<0>(p.red, r + u)));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            Acc v[NV];
            Tr::unpack(raw[u], v, conj);
                if constexpr (UN && !Tr::CX) un_apply_n<true, Acc, NV>(p.unA, v);
#pragma unroll
            for (int e = 0; e < NV; ++e) acc[e] = Tr::apply(op, acc[e], v[e]);
        }
    }
    for (; r < rEnd; ++r) {
        Acc v[NV];
        Tr::unpack(*reinterpret_cast<const wu32x4*>(A + rd_offset<0>(p.red, r)), v, conj);
        if constexpr (UN && !Tr::CX) un_apply_n<true, Acc, NV>(p.unA, v);
#pragma unroll
        for (int e = 0; e < NV; ++e) acc[e] = Tr::apply(op, acc[e], v[e]);
    }
    if (p.partial != nullptr) {
        Acc* P = static_cast<Acc*>(p.partial) + (size_t)split * p.kept.total + kv;
#pragma unroll
        for (int e = 0; e < NV; ++e) P[e] = acc[e];
        return;
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) w_finish<Tr, UN>(p, kv + e, acc[e]);
}

// one wave per (kept element, split): its lanes stride over the reduced range with 16-byte loads (reduced mode 0 is contiguous, its
// extent and redPerSplit multiples of NV) and meet through lane shuffles
template <class Tr>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(reduce_row_wide)(const ReduceParams p) {
    constexpr bool UN = CTAMD_UN;
    typedef typename Tr::Elem Elem;
    typedef typename Tr::Acc Acc;
    constexpr int NV = Tr::NV;
    constexpr uint32_t CH = 64u * NV;          // elements one wave-load covers
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (k >= p.kept.total) return;
    const int lane = threadIdx.x & 63;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * p.redPerSplit;
    uint32_t rEnd = rBegin + p.redPerSplit;
    if (rEnd > p.red.total) rEnd = p.red.total;
    const int op = p.op;
    const bool conj = Tr::CX && p.conjA != 0;
    const Elem* A = static_cast<const Elem*>(p.A) + rd_offset<0>(p.kept, k);
    Acc acc = Tr::identity(op);
    uint32_t r = rBegin + (uint32_t)NV * (uint32_t)lane;
    for (; r + 3u * CH < rEnd; r += 4u * CH) {
        wu32x4 raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) raw[u] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(A + rd_offset<0>(p.red, r + CH * u)));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            Acc v[NV];
            Tr::unpack(raw[u], v, conj);
                if constexpr (UN && !Tr::CX) un_apply_n<true, Acc, NV>(p.unA, v);
#pragma unroll
            for (int e = 0; e < NV; ++e) acc = Tr::apply(op, acc, v[e]);
        }
    }
    for (; r < rEnd; r += CH) {
        Acc v[NV];
        Tr::unpack(*reinterpret_cast<const wu32x4*>(A + rd_offset<0>(p.red, r)), v, conj);
        if constexpr (UN && !Tr::CX) un_apply_n<true, Acc, NV>(p.unA, v);
#pragma unroll
        for (int e = 0; e < NV; ++e) acc = Tr::apply(op, acc, v[e]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = Tr::apply(op, acc, Tr::shfl_down(acc, off));
    if (lane != 0) return;
    if (p.partial != nullptr) {
        static_cast<Acc*>(p.partial)[(size_t)split * p.kept.total + k] = acc;
        return;
    }
    w_finish<Tr, UN>(p, k, acc);
}

template <typename T, typename S>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(reduce_generic)(const ReduceParams p) {
    constexpr bool UN = CTAMD_UN;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= p.kept.total) return;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * p.redPerSplit;
    uint32_t rEnd = rBegin + p.redPerSplit;
    if (rEnd > p.red.total) rEnd = p.red.total;
    const int op = p.op;
    const T* A = static_cast<const T*>(p.A) + rd_offset<0>(p.kept, k);
    S acc = red_identity<S>(op);
    // (round 6: eight / four loads in flight per lane — the loop used to issue one load and wait for it, 1.5 TB/s on 'abc->ac' at odd
    // extents where neighbouring lanes DO read neighbouring elements; same order of the combines, same bits)
    uint32_t r = rBegin;
    if (p.red.n == 1) {
        const int64_t step = p.red.stride[0][0];
        const T* q = A + (int64_t)r * step;
        for (; r + 8 <= rEnd; r += 8, q += 8 * step) {
            S v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (S)rg_load<T>(q + (int64_t)u * step);
            un_apply_n<UN, S, 8>(p.unA, v);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = red_apply<S>(op, acc, v[u]);
        }
    }
    for (; r + 4 <= rEnd; r += 4) {
        S v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (S)rg_load<T>(A + rd_offset<0>(p.red, r + u));
        un_apply_n<UN, S, 4>(p.unA, v);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = red_apply<S>(op, acc, v[u]);
    }
    for (; r < rEnd; ++r) acc = red_apply<S>(op, acc, un_apply<UN, S>(p.unA, (S)rg_load<T>(A + rd_offset<0>(p.red, r))));
    if (p.partial != nullptr) {
        static_cast<S*>(p.partial)[(size_t)split * p.kept.total + k] = acc;
        return;
    }
    const S alpha = sizeof(S) == 8 ? (S)p.alpha64 : (S)p.alpha;
    const S beta  = sizeof(S) == 8 ? (S)p.beta64 : (S)p.beta;
    S val = alpha * acc;
    if (beta != (S)0) val += beta * un_apply<UN, S>(p.unC, (S)rg_load<T>(static_cast<const T*>(p.C) + rd_offset<2>(p.kept, k)));
    rg_store<T>(static_cast<T*>(p.D) + rd_offset<1>(p.kept, k), (double)val);
}

// RED_GENERIC with A's stride-1 mode REDUCED (ReduceParams::rowAny, round 6): 'abc->bc', 'ab->b' at extents / alignments the 16-byte-lane
// row kernel refuses.  One lane per kept element (above) puts neighbouring lanes a kept stride apart — 0.4-0.6 TB/s; here one WAVE owns a
// kept element, its lanes stride over the reduced range element by element (coalesced), four loads in flight, and meet through lane
// shuffles.  Partials as above ([splitR][kept] accumulators).
template <typename T, typename S>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(reduce_row_any)(const ReduceParams p) {
    constexpr bool UN = CTAMD_UN;
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (k >= p.kept.total) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t split = blockIdx.y;
    const uint32_t rBegin = split * p.redPerSplit;
    uint32_t rEnd = rBegin + p.redPerSplit;
    if (rEnd > p.red.total) rEnd = p.red.total;
    const int op = p.op;
    const T* A = static_cast<const T*>(p.A) + rd_offset<0>(p.kept, k);
    S acc = red_identity<S>(op);
    uint32_t r = rBegin + lane;
    for (; r + 3u * 64u < rEnd; r += 4u * 64u) {
        S v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (S)rg_load<T>(A + rd_offset<0>(p.red, r + 64u * (uint32_t)u));
        un_apply_n<UN, S, 4>(p.unA, v);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = red_apply<S>(op, acc, v[u]);
    }
    for (; r < rEnd; r += 64u) acc = red_apply<S>(op, acc, un_apply<UN, S>(p.unA, (S)rg_load<T>(A + rd_offset<0>(p.red, r))));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = red_apply<S>(op, acc, __shfl_down(acc, off, 64));
    if (lane != 0u) return;
    if (p.partial != nullptr) {
        static_cast<S*>(p.partial)[(size_t)split * p.kept.total + k] = acc;
        return;
    }
    const S alpha = sizeof(S) == 8 ? (S)p.alpha64 : (S)p.alpha;
    const S beta  = sizeof(S) == 8 ? (S)p.beta64 : (S)p.beta;
    S val = alpha * acc;
    if (beta != (S)0) val += beta * un_apply<UN, S>(p.unC, (S)rg_load<T>(static_cast<const T*>(p.C) + rd_offset<2>(p.kept, k)));
    rg_store<T>(static_cast<T*>(p.D) + rd_offset<1>(p.kept, k), (double)val);
}

// D[k] = alpha * combine_s partial[s][k] + beta * unC(C[k])      (the partials already hold unA(A): no operator on them)
template <typename T, typename S>
__global__ void __launch_bounds__(256) CTAMD_KERNEL(reduce_finalize)(const ReduceParams p) {
    constexpr bool UN = CTAMD_UN;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= p.kept.total) return;
    const int op = p.op;
    const S* P = static_cast<const S*>(p.partial) + k;
    S acc = red_identity<S>(op);
    for (uint32_t s = 0; s < p.splitR; ++s) acc = red_apply<S>(op, acc, P[(size_t)s * p.kept.total]);
    const S alpha = sizeof(S) == 8 ? (S)p.alpha64 : (S)p.alpha;
    const S beta  = sizeof(S) == 8 ? (S)p.beta64 : (S)p.beta;
    S val = alpha * acc;
    if (beta != (S)0) val += beta * un_apply<UN, S>(p.unC, (S)rg_load<T>(static_cast<const T*>(p.C) + rd_offset<2>(p.kept, k)));
    rg_store<T>(static_cast<T*>(p.D) + rd_offset<1>(p.kept, k), (double)val);
}
