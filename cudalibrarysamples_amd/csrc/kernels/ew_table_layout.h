// ew_table_layout.h — argument block and index arithmetic of the mode-table element-wise and reduction kernels
// (elementwise_table.hip): tensors of up to 64 modes, where the tile + four-digit "rest" decomposition of Ew2DParams / ReduceParams
// gives up.  Plain C++ (no HIP), so that the same functions are compiled into the kernels, into the planner
// (host/plan_elementwise_table.cpp) AND into a host harness that walks every tile and position of a table on the CPU
// (tests/harness/ew_table_layout_harness.cpp): every element of D must be produced exactly once, from the right offsets in A and C.
//
// The view of a problem: D's modes of extent > 1 after the planner's fusion, sorted by D's stride — at most 64.  The whole table
// travels BY VALUE in the kernel arguments (about 3.7 KiB of the 4-KiB argument block): cutensorPermute has no workspace parameter and
// plans are made on machines without a GPU, so a plan owns no device memory.  Every function takes the table through a pointer type
// of the caller's choice: a plain pointer on the host, a pointer into the constant address space — the kernel-argument segment itself
// — on the device, where indexing a by-value struct with a run-time index would make the compiler copy it into scratch.
//
// Three kernels read the block, each its own part of it:
//   * tile kernel   — mode[0, nEntries) is the OUTER index of a tile (fastest first): the modes outside the tile, and for each CUT tile
//                     mode the index of its piece; tileA[] / tileD[] list the tile modes in A's and in D's stride order.
//   * gather kernel — mode[0, nEntries) are all modes of the view in D's order; one output element = one index over them.
//   * reduction     — mode[0, nKept) the kept modes in D's order, mode[nKept, nKept + nRed) the reduced ones in A's order (sA only).
// Offsets inside a tile are 32-bit (the planner sends a problem whose tile spans 2^31 elements or more in A, D or C to the gather
// kernel); every offset that multiplies a digit of the outer / gather / reduction index by a stride is 64-bit.
#pragma once
#include <stdint.h>

#include "params.h"

#if defined(__HIPCC__)
#define CTAMD_HD __host__ __device__ __forceinline__
#else
#define CTAMD_HD inline
#endif

namespace ctamd {

constexpr int kEwTableMaxModes = 64;      // what cutensorCreateTensorDescriptor accepts
constexpr int kEwTableMaxTileModes = 16;  // per stride order; a tile takes at most 7 modes from each side (2^7 two-byte elements = 256 bytes)
constexpr int kEwTableThreads = 256;
// A tile has at most 2048 positions of 2- or 4-byte elements, 1024 of 8- or 16-byte elements — 8 / 4 per thread: their tile-relative
// offsets (five words each) and the elements in flight stay inside 128 registers a lane, the operator twins and the complex arithmetic
// included.  That is 4 / 8 / 8 / 16 KiB of LDS: the budget is 16 KiB.
constexpr uint32_t kEwTableLdsBytes = 16384;
constexpr uint32_t ew_table_positions(uint32_t elemBytes) { return elemBytes <= 4u ? 2048u : 1024u; }
// what the tile kernel of an element size declares: the planner's figure in the plan's description ("lds")
constexpr uint32_t ew_table_lds_bytes(uint32_t elemBytes) { return ew_table_positions(elemBytes) * elemBytes; }
// run of contiguous bytes a tile aims for on each side
constexpr uint32_t kEwTableRunBytes = 256;

enum EwTableKind : uint32_t { EWT_TILE = 0, EWT_GATHER = 1, EWT_REDUCE = 2 };

struct EwTableMode {
    FastDiv  div;            // extent (outer entry of a cut mode: its number of pieces)
    uint32_t cut;            // tile kernel: 0 — a mode outside the tile; 1 / 2 — the piece index of cut mode 0 / 1
    int64_t  sA, sD, sC;     // element strides (cut entry: times the piece length)
};
static_assert(sizeof(EwTableMode) == 40, "64 entries are 2.5 KiB");

struct EwTileMode {
    FastDiv  div;            // extent of the mode INSIDE a tile (the piece length of a cut mode)
    uint32_t cut;            // 0, or 1 / 2: this mode is cut mode 0 / 1 (its digit is compared with the piece's live length)
    uint32_t sA, sD, sC;     // element strides
    uint32_t rankA;          // tileD[] only: what one step of this mode adds to the position's rank in A's order
};
static_assert(sizeof(EwTileMode) == 32, "2 x 16 entries are 1 KiB");

struct EwTable {
    const void* A;
    const void* C;           // null: C is not read
    void*       D;
    void*       partial;     // reduction: [splitR][keptTotal] accumulators, or null
    double      alpha64, alphaIm, gamma64, gammaIm;   // gamma: the scalar of C (a reduction's beta)
    int32_t     opAC;        // combiner of alpha A with gamma C (cutensorOperator_t; reductions: ADD)
    int32_t     opReduce;    // reduction operator
    int32_t     conjA, conjC;
    uint8_t     unA, unC;    // unary operators on real data (unary_op.h)
    uint32_t    kind;        // EwTableKind
    uint32_t    nModes;      // modes of the view (the description's "modes")
    uint32_t    nEntries;    // entries of mode[] the kernel walks
    uint32_t    total;       // tile kernel: tiles; gather kernel: elements of D; reduction: kept elements   (< 2^31)
    // tile kernel
    uint32_t    nTileA, nTileD;       // entries of tileA[] / tileD[] (the same set of modes in two orders)
    uint32_t    tilePos;              // positions of a tile = product of the tile extents
    uint32_t    cutExtent[2];         // full extent of cut mode 0 / 1 (0: no such cut mode)
    uint32_t    cutPiece[2];          // its piece length
    // reduction
    uint32_t    nKept, nRed;
    uint32_t    redTotal, splitR, redPerSplit;
    EwTileMode  tileA[kEwTableMaxTileModes];
    EwTileMode  tileD[kEwTableMaxTileModes];
    EwTableMode mode[kEwTableMaxModes];
};
static_assert(sizeof(EwTable) <= 4096, "the table travels in the 4-KiB kernel-argument block");

// n / d for n < 2^31 (FastDiv of params.h; d = 1 divides by nothing)
CTAMD_HD uint32_t ewt_div(uint32_t n, uint32_t d, uint32_t magic, uint32_t shift) {
    return d < 2u ? n : (uint32_t)(((uint64_t)n * magic) >> 32) >> shift;
}

// LDS slot of the position with rank r in A's order.  The tile is parked in A's order and read back in D's: consecutive lanes of the
// read then differ in HIGH bits of r (a reversal of extent-2 modes is a bit reversal) — all on one bank as they stand.  The slot folds
// the rank's bits 5-9 and 10-11 onto its low five: lanes that differ only inside one of the three groups keep distinct banks, and the
// write side (consecutive ranks, high bits equal) stays a permutation of each 32-slot row.
CTAMD_HD uint32_t ewt_slot(uint32_t r) { return r ^ ((r >> 5) & 31u) ^ ((r >> 10) & 3u); }

struct EwtOrigin {
    int64_t  oA, oD, oC;     // element offsets of the tile's first position
    uint32_t live0, live1;   // live length of cut mode 0 / 1 in this tile (the piece length, less in a mode's last piece)
};
// the outer index of tile `t`, decoded once per tile
template <class Tab>
CTAMD_HD EwtOrigin ewt_tile_origin(Tab tab, uint32_t t) {
    EwtOrigin o;
    o.oA = o.oD = o.oC = 0;
    o.live0 = o.live1 = 0xffffffffu;          // (no cut mode: every digit is live)
    const uint32_t n = tab->nEntries;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t d = tab->mode[i].div.d;
        const uint32_t q = ewt_div(t, d, tab->mode[i].div.magic, tab->mode[i].div.shift);
        const uint32_t digit = t - q * d;
        t = q;
        o.oA += (int64_t)digit * tab->mode[i].sA;
        o.oD += (int64_t)digit * tab->mode[i].sD;
        o.oC += (int64_t)digit * tab->mode[i].sC;
        const uint32_t cut = tab->mode[i].cut;
        if (cut != 0u) {
            const uint32_t piece = tab->cutPiece[cut - 1u], left = tab->cutExtent[cut - 1u] - digit * piece;
            const uint32_t live = left < piece ? left : piece;
            if (cut == 1u) o.live0 = live; else o.live1 = live;
        }
    }
    return o;
}

// a position's digits of the two cut modes, packed: digit of cut mode 0 | digit of cut mode 1 << 8 (a piece is at most 256 long)
CTAMD_HD bool ewt_live(uint32_t cuts, uint32_t live0, uint32_t live1) { return (cuts & 0xffu) < live0 && ((cuts >> 8) & 0xffu) < live1; }

struct EwtPosA { uint32_t relA, cuts; };
// position with rank r in A's order (consecutive r = consecutive addresses of A): its offset in A relative to the tile's origin
template <class Tab>
CTAMD_HD EwtPosA ewt_pos_a(Tab tab, uint32_t r) {
    EwtPosA p{0u, 0u};
    const uint32_t n = tab->nTileA;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t d = tab->tileA[i].div.d;
        const uint32_t q = ewt_div(r, d, tab->tileA[i].div.magic, tab->tileA[i].div.shift);
        const uint32_t digit = r - q * d;
        r = q;
        p.relA += digit * tab->tileA[i].sA;
        const uint32_t cut = tab->tileA[i].cut;
        if (cut != 0u) p.cuts |= digit << (8u * (cut - 1u));
    }
    return p;
}

struct EwtPosD { uint32_t relD, relC, rankA, cuts; };
// position with rank r in D's order: its offsets in D and C relative to the tile's origin and its rank in A's order (where it was parked)
template <class Tab>
CTAMD_HD EwtPosD ewt_pos_d(Tab tab, uint32_t r) {
    EwtPosD p{0u, 0u, 0u, 0u};
    const uint32_t n = tab->nTileD;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t d = tab->tileD[i].div.d;
        const uint32_t q = ewt_div(r, d, tab->tileD[i].div.magic, tab->tileD[i].div.shift);
        const uint32_t digit = r - q * d;
        r = q;
        p.relD += digit * tab->tileD[i].sD;
        p.relC += digit * tab->tileD[i].sC;
        p.rankA += digit * tab->tileD[i].rankA;
        const uint32_t cut = tab->tileD[i].cut;
        if (cut != 0u) p.cuts |= digit << (8u * (cut - 1u));
    }
    return p;
}

struct EwtOffsets { int64_t oA, oD, oC; };
// every digit of index idx over mode[first, first + n): the gather kernel's element, a reduction's kept element (first = 0) or reduced
// element (first = nKept; only oA means something)
template <class Tab>
CTAMD_HD EwtOffsets ewt_offsets(Tab tab, uint32_t first, uint32_t n, uint32_t idx) {
    EwtOffsets o{0, 0, 0};
    for (uint32_t i = first; i < first + n; ++i) {
        const uint32_t d = tab->mode[i].div.d;
        const uint32_t q = ewt_div(idx, d, tab->mode[i].div.magic, tab->mode[i].div.shift);
        const uint32_t digit = idx - q * d;
        idx = q;
        o.oA += (int64_t)digit * tab->mode[i].sA;
        o.oD += (int64_t)digit * tab->mode[i].sD;
        o.oC += (int64_t)digit * tab->mode[i].sC;
    }
    return o;
}

}  // namespace ctamd
