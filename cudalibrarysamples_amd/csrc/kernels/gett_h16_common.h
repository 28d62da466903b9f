// gett_h16_common.h — shared pieces of the 16-bit GETT kernels (gett_h16v.hip, gett_h16p.hip; gett_h16.hip holds their table): types, the
// operand staging tables (HOperand), the epilogue and the table slot of a retired family.  The LDS-DMA / fragment-read primitives and the K
// odometer are in gett_h16x_common.h.
//
// LDS image of an operand's K-tile (64 k): half-tiles of 128 rows = 16 KiB, staged by LDS-DMA (buffer_load_dwordx4 ... lds, 1 KiB per
// wave-instruction).  Which 16-byte unit of the half-tile a lane fetches is free, so the image is shaped by permuting the *source* units:
//   - K-contiguous operand (LAY_K): image [128 rows][64 k] (128-byte rows); unit p of row r holds k-unit p ^ ((r >> 1) & 7): the
//     ds_read_b128 fragment reads are conflict-free;
//   - free-contiguous operand (LAY_F): image [64 k][128 rows] (256-byte k-rows); unit p of k-row k holds row-unit
//     p ^ 4 (k & 3) ^ 2 ((k >> 3) & 1); fragments are read with the transposing ds_read_b64_tr_b16 (x_offF, gett_h16x_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "params.h"
#include "launch.h"
#include "gett_common.h"
#include "round16.h"

namespace ctamd {

constexpr int kHBK   = 64;            // K-tile
constexpr int kHTile = 256;           // BM = BN
constexpr int kHalfBytes = 16384;     // one half-tile: 128 rows x 64 k x 2 B

typedef short    s16x4 __attribute__((ext_vector_type(4)));
typedef short    s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16   bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float    f32x16 __attribute__((ext_vector_type(16)));

// Raw buffer descriptor (stride 0, num_records 2^32 - 1, gfx9 raw-buffer format word), built from
// readfirstlane'd words so that the compiler knows it is wave-uniform: an inline-asm "s" operand that is
// not provably uniform is silently given VGPRs.
typedef int HRsrc __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t h_uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// Minimum over the 64 lanes of a wave (all active) of byte offsets that lie within 2^31 of each other (the planner admits the
// 16-bit kernels only when ONE tile spans less than 2^31 bytes): the 32-bit differences to the first lane's value are reduced with
// four DPP steps inside each row of 16 lanes and four v_readlane — ~50 cycles.  (As six __shfl_xor rounds on 64-bit values this was
// 24 dependent ds_bpermute per kernel start, ~2.5k cycles of every workgroup's prologue: in-kernel stamps)
__device__ __forceinline__ int64_t h_wave_min(int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t ref = (int64_t)h_uniform64((uint64_t)v);
    int d = (int)(v - ref);
    int t;
    t = __builtin_amdgcn_update_dpp(d, d, 0xB1, 0xF, 0xF, false);  d = t < d ? t : d;     // quad_perm [1,0,3,2]
    t = __builtin_amdgcn_update_dpp(d, d, 0x4E, 0xF, 0xF, false);  d = t < d ? t : d;     // quad_perm [2,3,0,1]
    t = __builtin_amdgcn_update_dpp(d, d, 0x141, 0xF, 0xF, false); d = t < d ? t : d;     // row_half_mirror
    t = __builtin_amdgcn_update_dpp(d, d, 0x140, 0xF, 0xF, false); d = t < d ? t : d;     // row_mirror: every lane holds its row's minimum
    const int r0 = __builtin_amdgcn_readlane(d, 0), r1 = __builtin_amdgcn_readlane(d, 16);
    const int r2 = __builtin_amdgcn_readlane(d, 32), r3 = __builtin_amdgcn_readlane(d, 48);
    const int m01 = r0 < r1 ? r0 : r1, m23 = r2 < r3 ? r2 : r3;
    return ref + (int64_t)(m01 < m23 ? m01 : m23);
#else
    return v;
#endif
}

#define CTAMD_H_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define CTAMD_H_LGKM0()  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

template <bool BF>
__device__ __forceinline__ f32x16 h_mfma(s16x8 a, s16x8 b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else              return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
#else
    (void)a; (void)b; return c;
#endif
}

__device__ __forceinline__ float h_to_float(uint16_t v, bool bf) {
    if (bf) return __uint_as_float((uint32_t)v << 16);
    return (float)__builtin_bit_cast(_Float16, v);
}
__device__ __forceinline__ uint16_t h_from_float(float f, bool bf) {
    if (bf) {   // round to nearest even; NaN stays NaN
        uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
    return __builtin_bit_cast(uint16_t, (_Float16)f);
}

// ---------------------------------------------------------------------------------------------------------------------
// Epilogue of the 16-bit kernels: D = alpha * acc + beta * C, one rounding to the 16-bit type.
// An MFMA accumulator fragment holds one output column per lane (32 consecutive n in lanes 0-31, 16 rows in the 16
// registers).  Storing it from the registers means 16 two-byte stores per lane and fragment (two-byte stores cost ~12x the
// time per byte of 16-byte ones), and — worse — fully unrolled address arithmetic and conversions for every one of them:
// the first form of this epilogue was 100+ KB of straight-line code that every workgroup streamed through once, and the
// instruction fetch alone cost 30 us of a workgroup's 150 us on 8192^3 (K-sweep: 37 us fixed cost per workgroup, 7 us
// without the epilogue).  Now a wave parks four fragments at a time in 16 KiB of LDS of its own (the operand ring is dead by
// then: 64 ds_write_b32 in accumulator order, the only unrolled part) and a ROLLED loop of eight iterations turns them into
// 16-byte row pieces: every lane reads 8 consecutive n of one row, adds beta * C, converts (v_cvt_pk_bf16_f32 / v_cvt_f16_f32)
// and issues one 16-byte global store (rows of 64 contiguous bytes, 4 lanes each).  The vector form needs 8 consecutive n
// contiguous and 16-byte aligned in D (and in C when beta != 0): checked once per workgroup (wave-uniform); otherwise a rolled
// element-wise loop stores from the same LDS image with any strides.
// ---------------------------------------------------------------------------------------------------------------------
// h_round16 / h_round16_with_c: round16.h (shared with the split-K folds, the general family and gett_simple.hip)
template <bool BF>
__device__ __forceinline__ s16x8 h_round8(const f32x4& v0, const f32x4& v1) {
    return s16x8{(short)h_round16<BF>(v0[0]), (short)h_round16<BF>(v0[1]), (short)h_round16<BF>(v0[2]), (short)h_round16<BF>(v0[3]),
                 (short)h_round16<BF>(v1[0]), (short)h_round16<BF>(v1[1]), (short)h_round16<BF>(v1[2]), (short)h_round16<BF>(v1[3])};
}
template <bool BF>
__device__ __forceinline__ s16x8 h_round8_with_c(const f32x4& v0, const f32x4& v1, float beta, const s16x8& cv) {
    return s16x8{(short)h_round16_with_c<BF>(v0[0], beta, (uint16_t)cv[0]), (short)h_round16_with_c<BF>(v0[1], beta, (uint16_t)cv[1]),
                 (short)h_round16_with_c<BF>(v0[2], beta, (uint16_t)cv[2]), (short)h_round16_with_c<BF>(v0[3], beta, (uint16_t)cv[3]),
                 (short)h_round16_with_c<BF>(v1[0], beta, (uint16_t)cv[4]), (short)h_round16_with_c<BF>(v1[1], beta, (uint16_t)cv[5]),
                 (short)h_round16_with_c<BF>(v1[2], beta, (uint16_t)cv[6]), (short)h_round16_with_c<BF>(v1[3], beta, (uint16_t)cv[7])};
}

// C and D are device memory: the epilogues address them through the GLOBAL address space (global_load / global_store), not through
// generic pointers (flat_*).  A flat operation "may touch LDS" for the compiler's wait-count bookkeeping: inside a kernel that loops
// over tiles (gett_h16p.hip) one pending flat store turned every counted LDS wait of the main loop into lgkmcnt(0).
typedef s16x8 __attribute__((address_space(1))) * HGlbS8;
typedef const s16x8 __attribute__((address_space(1))) * HGlbCS8;
typedef uint16_t __attribute__((address_space(1))) * HGlbU16;
typedef const uint16_t __attribute__((address_space(1))) * HGlbCU16;

struct HEpilogue {
    const uint16_t* C;
    uint16_t*       D;
    float alpha, beta;
    uint32_t Mtot, Ntot;
    bool vecD, vecC;
    bool flat;           // M and N are single modes: offsets are one multiplication, no digit decomposition
    float* scratch;      // this wave's 16 KiB of LDS: four fragments [32 rows][32 n] fp32

    __device__ __forceinline__ void init(const GettParams& p, uint32_t l, char* lds, int wave, int bytesPerWave = 16384) {
        C = static_cast<const uint16_t*>(p.C);
        D = static_cast<uint16_t*>(p.D);
        int64_t oD, oC;
        group_offset2<2>(p.gL, p.cStrideL, l, oD, oC);
        D += oD;
        C += oC;
        alpha = p.alpha; beta = p.beta;
        Mtot = p.gM.total; Ntot = p.gN.total;
        scratch = reinterpret_cast<float*>(lds + wave * bytesPerWave);
        // 16-byte chunks: 8 consecutive n are contiguous and stay inside the fastest N mode — its extent is a multiple of 8, or it is
        // the ONLY N mode (then a row's last chunk may be partial: store16 / load16 below).  No alignment condition (round 6): a
        // 16-byte global access works at any 2-byte address (tools/ubench/ldsdma_unaligned.hip), so a row pitch of 4100 or 4097
        // elements keeps the chunk path instead of 2-byte stores (~12x the time per byte).
        const bool d = p.gN.stride[1][0] == 1 && (p.gN.n <= 1 || p.gN.div[0].d % 8u == 0u);
        vecD = d;
        vecC = d && p.cStrideN[0] == 1;
        flat = p.gM.n <= 1 && p.gN.n <= 1;
    }
    __device__ __forceinline__ void offsets(const GettParams& p, uint32_t m, uint32_t n, int64_t& offD, int64_t& offC) const {
        if (flat) {
            offD = (int64_t)m * p.gM.stride[1][0] + (int64_t)n * p.gN.stride[1][0];
            offC = (int64_t)m * p.cStrideM[0] + (int64_t)n * p.cStrideN[0];
        } else {
            int64_t dm, cm, dn, cn;
            group_offset2<1>(p.gM, p.cStrideM, m, dm, cm);
            group_offset2<1>(p.gN, p.cStrideN, n, dn, cn);
            offD = dm + dn; offC = cm + cn;
        }
    }

    // One 16-byte chunk (columns n .. n + 7 of a row) to D / from C.  A chunk that sticks out of a ragged N mode (n + 8 > Ntot: one N
    // mode, extent % 8 != 0) moves the columns that exist, one element at a time: nothing is read or written past the row.
    __device__ __forceinline__ void store16(uint16_t* dst, const s16x8& v, uint32_t n) const {
        if (n + 8u <= Ntot) { __builtin_nontemporal_store(v, (HGlbS8)(uintptr_t)dst); return; }
#define CTAMD_EP_ST1(E) if (n + (E) < Ntot) *(HGlbU16)(uintptr_t)(dst + (E)) = (uint16_t)v[E];
        CTAMD_EP_ST1(0) CTAMD_EP_ST1(1) CTAMD_EP_ST1(2) CTAMD_EP_ST1(3) CTAMD_EP_ST1(4) CTAMD_EP_ST1(5) CTAMD_EP_ST1(6)
#undef CTAMD_EP_ST1
    }
    __device__ __forceinline__ s16x8 load16(const uint16_t* src, uint32_t n) const {
        if (n + 8u <= Ntot) return *(HGlbCS8)(uintptr_t)src;
        s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#define CTAMD_EP_LD1(E) if (n + (E) < Ntot) v[E] = (short)*(HGlbCU16)(uintptr_t)(src + (E));
        CTAMD_EP_LD1(0) CTAMD_EP_LD1(1) CTAMD_EP_LD1(2) CTAMD_EP_LD1(3) CTAMD_EP_LD1(4) CTAMD_EP_LD1(5) CTAMD_EP_LD1(6)
#undef CTAMD_EP_LD1
        return v;
    }

    // ---- beta != 0 with 16-byte lanes in C and D, one chunk at a time (gett_h16w4x_kernel's pipelined beta path) ----------------------
    // chunk IT (0 .. 7) of a pass of four parked 32 x 32 fragments (the layout of flush<.., NF = 4> below): fragment IT >> 1, 16-byte
    // chunk (IT & 1) * 64 + lane of its 128.  Compile-time chunk numbers and caller-named registers: an array of chunks indexed by a
    // loop variable is a stack object whenever the unroller gives up, and scratch is paid for at every dispatch.
    template <int IT>
    __device__ __forceinline__ void chunk_coords(uint32_t mB0, uint32_t nB0, uint32_t nHi, uint32_t nLo, int lane, uint32_t& m, uint32_t& n, int& ldsFloat) const {
        constexpr int f = IT >> 1;
        const uint32_t nB = nB0 + nHi * (uint32_t)(f >> 1) + nLo * (uint32_t)(f & 1);
        const int cidx = lane + 64 * (IT & 1), row = cidx >> 2, piece = cidx & 3;
        m = mB0 + (uint32_t)row;
        n = nB + 8u * (uint32_t)piece;
        ldsFloat = f * 1024 + row * 32 + piece * 8;
    }
    template <int IT>
    __device__ __forceinline__ void load_c_chunk(const GettParams& p, uint32_t mB0, uint32_t nB0, uint32_t nHi, uint32_t nLo, int lane, s16x8& cv) const {
        uint32_t m, n;
        int at;
        chunk_coords<IT>(mB0, nB0, nHi, nLo, lane, m, n, at);
        if (m < Mtot && n < Ntot) {
            int64_t offD, offC;
            offsets(p, m, n, offD, offC);
            cv = load16(C + offC, n);
        }
    }
    template <bool BF, int IT>
    __device__ __forceinline__ void store_chunk_with_c(const GettParams& p, uint32_t mB0, uint32_t nB0, uint32_t nHi, uint32_t nLo, int lane, const s16x8& cv) const {
        uint32_t m, n;
        int at;
        chunk_coords<IT>(mB0, nB0, nHi, nLo, lane, m, n, at);
        f32x4 v0 = *reinterpret_cast<const f32x4*>(scratch + at);
        f32x4 v1 = *reinterpret_cast<const f32x4*>(scratch + at + 4);
        if (m < Mtot && n < Ntot) {
            int64_t offD, offC;
            offsets(p, m, n, offD, offC);
            const s16x8 out = h_round8_with_c<BF>(v0, v1, beta, cv);
            store16(D + offD, out, n);
        }
    }

    // ---- four-fragment form ---------------------------------------------------------------------------------------------
    // store the four parked fragments; fragment f covers rows mB + mHi (f >> 1) + mLo (f & 1) + [0, 32), columns alike
    // (base + steps, not arrays of four: a runtime-indexed array lands on the stack, and a scratch allocation is paid for at
    // every dispatch)
    // NF: fragments parked (4; 1: fragment 0 only — the 64 x 64 kernel's one fragment per wave)
    template <bool BF, int NF = 4>
    __device__ __forceinline__ void flush(const GettParams& p, uint32_t mB0, uint32_t mHi, uint32_t mLo, uint32_t nB0, uint32_t nHi, uint32_t nLo, int lane) const {
        if (vecD) {
#pragma unroll 2
            for (int it = 0; it < 2 * NF; ++it) {         // fragment it >> 1, chunks (it & 1) * 64 + lane of its 128
                const int f = it >> 1;
                const uint32_t mB = mB0 + mHi * (uint32_t)(f >> 1) + mLo * (uint32_t)(f & 1);
                const uint32_t nB = nB0 + nHi * (uint32_t)(f >> 1) + nLo * (uint32_t)(f & 1);
                const int cidx = lane + 64 * (it & 1), row = cidx >> 2, piece = cidx & 3;
                const float* src = scratch + f * 1024 + row * 32 + piece * 8;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 4);
                const uint32_t m = mB + row, n = nB + 8 * piece;
                if (m < Mtot && n < Ntot) {
                    int64_t offD, offC;
                    offsets(p, m, n, offD, offC);
                    const f32x4 v0 = lo, v1 = hi;
                    s16x8 out;
                    if (beta != 0.f) {
                        s16x8 cv = {0, 0, 0, 0, 0, 0, 0, 0};     // explicit elements below: nothing here may become a stack array
                        if (vecC) cv = load16(C + offC, n);
                        else {                                    // C is gathered element by element (a column past the end contributes zero)
#define CTAMD_EP_CS(E) if (n + (E) < Ntot) { int64_t oD_, oC_; offsets(p, m, n + (E), oD_, oC_); cv[E] = (short)*(HGlbCU16)(uintptr_t)(C + oC_); }
                            CTAMD_EP_CS(0) CTAMD_EP_CS(1) CTAMD_EP_CS(2) CTAMD_EP_CS(3) CTAMD_EP_CS(4) CTAMD_EP_CS(5) CTAMD_EP_CS(6) CTAMD_EP_CS(7)
#undef CTAMD_EP_CS
                        }
                        out = h_round8_with_c<BF>(v0, v1, beta, cv);
                    } else out = h_round8<BF>(v0, v1);
                    store16(D + offD, out, n);   // nontemporal: the result is not read again by this kernel
                }
            }
            return;
        }
        // element-wise form (any strides): lane = column, one row per iteration
#pragma unroll 1
        for (int it = 0; it < NF * 32; ++it) {
            const int f = it >> 5, row = it & 31;
            const uint32_t mB = mB0 + mHi * (uint32_t)(f >> 1) + mLo * (uint32_t)(f & 1);
            const uint32_t nB = nB0 + nHi * (uint32_t)(f >> 1) + nLo * (uint32_t)(f & 1);
            if (lane < 32) {
                const uint32_t m = mB + row, n = nB + lane;
                if (m < Mtot && n < Ntot) {
                    int64_t offD, offC;
                    offsets(p, m, n, offD, offC);
                    float val = scratch[f * 1024 + row * 32 + lane];
                    *(HGlbU16)(uintptr_t)(D + offD) = (beta != 0.f) ? h_round16_with_c<BF>(val, beta, *(HGlbCU16)(uintptr_t)(C + offC)) : h_round16<BF>(val);
                }
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------
// One operand (A rows or B columns) of the streamed K-tile.
// ---------------------------------------------------------------------------------------------
// Free-contiguous image: unit p of k-row k holds row-unit p ^ 4 (k & 3) ^ 2 ((k >> 3) & 1) — the 16-row fragments of the 16x16x32 MFMA
// take 32 bytes of a k-row per 16-lane group, and without the second term the two groups that a transposing read serves together
// (k-rows 8 g + .. and 8 (g + 1) + ..) land on the same banks.
// NH: half-tiles of 128 rows this operand stages per K-tile (2: the 256-row tiles; 1: the 128 x 128 mid-size kernel).
template <int LAY, int NH = 2>
struct HOperand {
    static constexpr int NW = 4;              // waves that stage a half-tile
    static constexpr int kPieces = 16 / NW;   // 1-KiB pieces of a half-tile this wave stages
    // Byte offset of this lane's 16-byte unit, [half-tile][piece i of this wave], for the K-tile at k = 0 — relative to
    // `base`, the smallest such offset in the wave: a workgroup tile spans far less than 2^32 bytes whatever the size of
    // the tensor, and `base` (64 bits, wave-uniform) goes into the buffer descriptor.
    uint32_t src[NH][kPieces];
    uint64_t base;

    __device__ __forceinline__ void init(const ModeGroup& gFree, int64_t strideK0, uint32_t row0, int wave, int lane) {
        int64_t off[NH][kPieces];
        int64_t mn = INT64_MAX;
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int i = 0; i < kPieces; ++i) {
                const int c = wave + NW * i;                     // 1-KiB piece of the half-tile
                if constexpr (LAY == LAY_K) {
                    const int r = 8 * c + (lane >> 3), p = lane & 7;
                    const int u = p ^ ((r >> 1) & 7);
                    uint32_t row = row0 + 128 * h + r;
                    if (row >= gFree.total) row = gFree.total - 1;   // clamped rows feed outputs that are never stored
                    off[h][i] = (group_offset<0>(gFree, row) + 8 * u) * 2;
                } else {
                    const int kk = 4 * c + (lane >> 4), p = lane & 15;
                    const int u = p ^ (4 * ((lane >> 4) & 3)) ^ (2 * ((kk >> 3) & 1));
                    uint32_t row = row0 + 128 * h + 8 * u;
                    // a unit past the edge is clamped to the last one that holds rows of the mode (whole when extent % 8 == 0; a ragged
                    // extent — one M / N mode, pick_h16_choice — leaves a partial last unit whose dead rows feed outputs nobody stores)
                    if (row >= gFree.total) row = (gFree.total - 1u) & ~7u;
                    off[h][i] = (group_offset<0>(gFree, row) + (int64_t)kk * strideK0) * 2;
                }
                mn = off[h][i] < mn ? off[h][i] : mn;
            }
        const int64_t mnW = (int64_t)h_uniform64((uint64_t)h_wave_min(mn));
        base = (uint64_t)mnW;
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int i = 0; i < kPieces; ++i) src[h][i] = (uint32_t)(off[h][i] - mnW);
    }
};

// A table slot of a RETIRED family (gett_h16.hip: H16_W8 .. H16_W4R; gett_h16v.hip: H16_W4V).  Kernel indices are written into plan-cache
// files, so the merged table keeps its length and order: the slot keeps the tile numbers, name and variant its entry always had, with
// `ablation` = 2 ("not built", skipped by rank_h16_choices) and a launcher that answers hipErrorNotSupported.
inline hipError_t launch_h16_not_built(const GettParams&, hipStream_t) { return hipErrorNotSupported; }
#define CTAMD_H16_RETIRED(bk, wn, threads, pf, la, lb, kname, variant) \
    {kHTile, kHTile, bk, 2, wn, 1, la, lb, threads, pf, 1, 2, &launch_h16_not_built, 0, 0, 0, 0, kname, variant},
// eight entries per family: bf16 first, then fp16, each in the order (layA, layB) = (K,K) (K,F) (F,K) (F,F)
#define CTAMD_H16_RETIRED8(bk, wn, threads, pf, kname, variant)                                                                               \
    CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_K, LAY_K, kname, variant) CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_K, LAY_F, kname, variant) \
    CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_F, LAY_K, kname, variant) CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_F, LAY_F, kname, variant) \
    CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_K, LAY_K, kname, variant) CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_K, LAY_F, kname, variant) \
    CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_F, LAY_K, kname, variant) CTAMD_H16_RETIRED(bk, wn, threads, pf, LAY_F, LAY_F, kname, variant)

// (h_reload_params: gett_common.h reload_params)
__device__ __forceinline__ void h_reload_params(GettParams& q) { reload_params(q); }

}  // namespace ctamd
