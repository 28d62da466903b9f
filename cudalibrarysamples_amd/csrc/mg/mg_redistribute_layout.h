// Index arithmetic of the block-cyclic redistribution (cutensorMgCopy): plain C++, included by the device code
// (mg_redistribute.hip), by the host plan (mg_copy.cpp) and, through ctamdMgCopyReplayOnHost, replayed by the CPU tests.
//
// A launch fills destination cells.  Every thread body below is written against (block index, thread index) arguments instead of
// the HIP builtins, so the kernels are one-line wrappers and the host replay runs the SAME decomposition — which lane touches which
// element, which run or tile it belongs to — thread by thread over host memory.
//
// Storage (cutensorMgCreateTensorDescriptor): index i of a mode lies in block b = i / blockSize at w = i % blockSize; the block
// belongs to grid coordinate b % deviceCount and is local block b / deviceCount of that cell; the element sits at
// w * elementStride + localBlock * blockStride (summed over modes) of the cell buffer; cells are linearised first mode fastest.
//
// The map runs from the DESTINATION: a destination cell's local coordinate l of a mode (l = localBlock * blockSize + w, l below
// dLocal = localBlocks * blockSize) gives the global index, which is valid below the extent (padding of ragged extents is skipped:
// never written, and nothing is read for it), and the global index gives the source cell and offset.  Cell index and offsets are
// sums over modes, so a mode's contribution (MgrPart) is computed where that mode's coordinate is fixed: once per row (rows form),
// once per tile edge (tile form).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MGR_HD __host__ __device__ inline
#else
#define MGR_HD inline
#endif

constexpr int kMgrMaxModes = 16;    // mode cap of cutensorMgCopy (blog_post.cu's tensors have up to 12)
constexpr int kMgrArgCells = 128;   // cells whose pointers travel in the kernel arguments; more go through the device workspace
constexpr int kMgrTile = 64;        // tile edge of the transposing form, in elements
constexpr int kMgrPitch = 65;       // LDS words per tile row: one word of padding (column reads then step 65 = 1 mod 32 banks;
                                    // 8-byte words: 130 dwords = 2 mod 64, conflict-free for the 32-lane groups of 64-bit reads)
constexpr int kMgrThreads = 256;

enum MgrForm : int32_t { MGR_FLAT = 0, MGR_ROWS = 1, MGR_TILE = 2, MGR_GATHER = 3 };

struct MgrMode {                    // one label, at its position in the DESTINATION's mode order
    uint32_t extent;
    uint32_t dBlock, dCount, dCellStride, dLocal;   // dLocal = localBlocks * blockSize: local coordinates of a destination cell
    uint32_t sBlock, sCount, sCellStride;
    int64_t dElemStride, dBlockStride, sElemStride, sBlockStride;
};

struct MgrArgs {
    MgrMode mode[kMgrMaxModes];
    const void* src[kMgrArgCells];  // every source cell                     (inline tables; unused when the *W pointers are set)
    void* dst[kMgrArgCells];        // the launch's destination cells, by slot
    int32_t dcell[kMgrArgCells];    // ... and their cell indices (the grid coordinates come from them)
    const void* const* srcW;        // the same three tables in the device workspace (more than kMgrArgCells cells), else null
    void* const* dstW;
    const int32_t* dcellW;
    uint64_t outer;                 // rows: rows per cell; tile: outer rows per cell; gather: elements per cell (padded local spaces)
    uint64_t work;                  // rows: = outer; tile: tiles per cell; gather: = outer
    uint32_t units, lprLog2;        // rows: lane units per row, log2(lanes per row)
    uint32_t tilesX, tilesY;        // tile
    int32_t nModes, fast, fastX;    // rows: fast = the common stride-1 label; tile: fast = destination's (Y), fastX = source's (X)
    int32_t nCells;                 // destination cells of this launch (grid.y)
    uint32_t gridX;
};

struct MgrPart { int64_t dOff, sOff; uint32_t sCell; uint32_t index; bool valid; };

MGR_HD const void* mgr_src(const MgrArgs& a, uint32_t c) { return a.srcW != nullptr ? a.srcW[c] : a.src[c]; }
MGR_HD void* mgr_dst(const MgrArgs& a, uint32_t slot) { return a.dstW != nullptr ? a.dstW[slot] : a.dst[slot]; }
MGR_HD uint32_t mgr_dcell(const MgrArgs& a, uint32_t slot) { return (uint32_t)(a.dcellW != nullptr ? a.dcellW[slot] : a.dcell[slot]); }
MGR_HD uint32_t mgr_coord(const MgrMode& m, uint32_t cell) { return (cell / m.dCellStride) % m.dCount; }

// adds mode m's contribution at local coordinate `local` of a destination cell with grid coordinate `coord`; p.index = global index
MGR_HD void mgr_map(const MgrMode& m, uint32_t coord, uint32_t local, MgrPart& p) {
    const uint32_t lb = local / m.dBlock, w = local - lb * m.dBlock;
    const uint32_t i = (lb * m.dCount + coord) * m.dBlock + w;      // below 2^31: checked by the plan
    p.index = i;
    if (i >= m.extent) { p.valid = false; return; }
    const uint32_t sb = i / m.sBlock, sw = i - sb * m.sBlock;
    const uint32_t sl = sb / m.sCount, sc = sb - sl * m.sCount;
    p.dOff += (int64_t)w * m.dElemStride + (int64_t)lb * m.dBlockStride;
    p.sOff += (int64_t)sw * m.sElemStride + (int64_t)sl * m.sBlockStride;
    p.sCell += sc * m.sCellStride;
}

// contributions of every mode but skipA / skipB at row r of the cell's padded local space (first remaining mode fastest)
MGR_HD void mgr_row_base(const MgrArgs& a, uint32_t cell, uint64_t r, int skipA, int skipB, MgrPart& p) {
    p.dOff = 0; p.sOff = 0; p.sCell = 0; p.index = 0; p.valid = true;
    for (int k = 0; k < a.nModes; ++k) {
        if (k == skipA || k == skipB) continue;
        const MgrMode& m = a.mode[k];
        const uint64_t q = r / m.dLocal;
        const uint32_t local = (uint32_t)(r - q * m.dLocal);
        r = q;
        mgr_map(m, mgr_coord(m, cell), local, p);
        if (!p.valid) return;
    }
}

template <int ES> struct MgrWord;
template <> struct MgrWord<2> { typedef uint16_t T; typedef uint32_t L; };   // L: the LDS word of the tile form
template <> struct MgrWord<4> { typedef uint32_t T; typedef uint32_t L; };
template <> struct MgrWord<8> { typedef uint64_t T; typedef uint64_t L; };
struct alignas(16) MgrVec { uint32_t v[4]; };

// ---- rows: the stride-1 label is the same on both sides ----------------------------------------------------------------------
// A row is one line of a destination cell along that label: dLocal local coordinates, cut into lane units of V elements
// (V = 16 / ES: 16-byte lanes, or V = 1).  A unit never straddles a block edge of either side (the plan grants V > 1 only when
// both block sizes are multiples of V), so it lies in ONE run — the stretch between two consecutive block edges of either side —
// and its source is V consecutive elements.  The row's last unit may be cut by a ragged extent: its valid elements go one by one.
// A workgroup holds 256 >> lprLog2 rows of 1 << lprLog2 lanes each.
template <int ES, int V>
MGR_HD void mgr_rows_unit(const MgrArgs& a, uint32_t slot, const MgrPart& base, uint32_t coordFast, uint32_t u) {
    typedef typename MgrWord<ES>::T T;
    const MgrMode& m = a.mode[a.fast];
    MgrPart p = base;
    mgr_map(m, coordFast, u * V, p);
    if (!p.valid) return;
    const char* s = static_cast<const char*>(mgr_src(a, p.sCell)) + p.sOff * ES;
    char* d = static_cast<char*>(mgr_dst(a, slot)) + p.dOff * ES;
    const uint32_t left = m.extent - p.index;
    if (V > 1 && left >= (uint32_t)V) { *reinterpret_cast<MgrVec*>(d) = *reinterpret_cast<const MgrVec*>(s); return; }
    const uint32_t n = left < (uint32_t)V ? left : (uint32_t)V;
    for (uint32_t e = 0; e < n; ++e) reinterpret_cast<T*>(d)[e] = reinterpret_cast<const T*>(s)[e];
}

template <int ES, int V>
MGR_HD void mgr_rows_thread(const MgrArgs& a, uint32_t bx, uint32_t by, uint32_t tid) {
    const uint32_t cell = mgr_dcell(a, by);
    const uint32_t lpr = 1u << a.lprLog2, rowsPerWg = kMgrThreads >> a.lprLog2;
    const uint32_t lane = tid & (lpr - 1), sub = tid >> a.lprLog2;
    const uint32_t coordFast = mgr_coord(a.mode[a.fast], cell);
    for (uint64_t row = (uint64_t)bx * rowsPerWg + sub; row < a.outer; row += (uint64_t)a.gridX * rowsPerWg) {
        MgrPart base;
        mgr_row_base(a, cell, row, a.fast, -1, base);      // once per row
        if (!base.valid) continue;
        for (uint32_t u = lane; u < a.units; u += lpr) mgr_rows_unit<ES, V>(a, by, base, coordFast, u);
    }
}

// ---- gather: one element per lane through the whole map ------------------------------------------------------------------------
template <int ES>
MGR_HD void mgr_gather_thread(const MgrArgs& a, uint32_t bx, uint32_t by, uint32_t tid) {
    typedef typename MgrWord<ES>::T T;
    const uint32_t cell = mgr_dcell(a, by);
    for (uint64_t e = (uint64_t)bx * kMgrThreads + tid; e < a.outer; e += (uint64_t)a.gridX * kMgrThreads) {
        MgrPart p;
        mgr_row_base(a, cell, e, -1, -1, p);
        if (!p.valid) continue;
        static_cast<T*>(mgr_dst(a, by))[p.dOff] = static_cast<const T*>(mgr_src(a, p.sCell))[p.sOff];
    }
}

// ---- tile: the stride-1 labels differ ------------------------------------------------------------------------------------------
// X = the source's stride-1 label, Y = the destination's.  A tile is kMgrTile x kMgrTile local coordinates (x, y) of one
// destination cell at one outer row (all other modes fixed).  Three phases with a barrier between them:
//   edges  threads 0..63 map the tile's x coordinates, threads 64..127 its y coordinates, thread 128 the outer row: the address parts
//          are computed once per tile edge and kept in LDS (MgrTileEdges); a coordinate in the padding has sCell < 0
//   load   lane = x (consecutive source elements inside a source block: coalesced reads), the four waves take y = wave + 4 j
//   store  lane = y (consecutive destination elements inside a destination block: coalesced writes), x = wave + 4 j
// The tile may straddle block and cell boundaries of both sides: every edge entry carries its own cell and offsets.
struct MgrTileEdges {
    int64_t dOff[2 * kMgrTile], sOff[2 * kMgrTile];
    int32_t sCell[2 * kMgrTile];
    int64_t baseD, baseS;
    int32_t baseCell, pad;
};
// static LDS of the tile kernels: the tile [kMgrTile][kMgrPitch] in 4-byte words for 2- and 4-byte elements (16640 bytes), in
// 8-byte words for 8-byte elements (33280 bytes), plus the edges (2584 bytes): 19224 / 35864 bytes
constexpr int kMgrTileLds4 = kMgrTile * kMgrPitch * 4 + (int)sizeof(MgrTileEdges);
constexpr int kMgrTileLds8 = kMgrTile * kMgrPitch * 8 + (int)sizeof(MgrTileEdges);
static_assert(sizeof(MgrTileEdges) == 2584 && kMgrTileLds4 == 19224 && kMgrTileLds8 == 35864, "the LDS sizes the comment states");

MGR_HD void mgr_tile_split(const MgrArgs& a, uint64_t t, uint32_t& tx, uint32_t& ty, uint64_t& row) {
    tx = (uint32_t)(t % a.tilesX);
    t /= a.tilesX;
    ty = (uint32_t)(t % a.tilesY);
    row = t / a.tilesY;
}

MGR_HD void mgr_tile_edges(const MgrArgs& a, uint32_t by, uint64_t t, uint32_t tid, MgrTileEdges& e) {
    const uint32_t cell = mgr_dcell(a, by);
    uint32_t tx, ty;
    uint64_t row;
    mgr_tile_split(a, t, tx, ty, row);
    MgrPart p;
    if (tid < 2 * kMgrTile) {
        const bool isX = tid < kMgrTile;
        const MgrMode& m = a.mode[isX ? a.fastX : a.fast];
        const uint32_t local = (isX ? tx : ty) * kMgrTile + (tid & (kMgrTile - 1));
        p.dOff = 0; p.sOff = 0; p.sCell = 0; p.index = 0; p.valid = local < m.dLocal;
        if (p.valid) mgr_map(m, mgr_coord(m, cell), local, p);
        e.dOff[tid] = p.dOff; e.sOff[tid] = p.sOff; e.sCell[tid] = p.valid ? (int32_t)p.sCell : -1;
    } else if (tid == 2 * kMgrTile) {
        mgr_row_base(a, cell, row, a.fast, a.fastX, p);
        e.baseD = p.dOff; e.baseS = p.sOff; e.baseCell = p.valid ? (int32_t)p.sCell : -1;
    }
}

template <int ES>
MGR_HD void mgr_tile_load(const MgrArgs& a, uint32_t tid, const MgrTileEdges& e, typename MgrWord<ES>::L* tile) {
    typedef typename MgrWord<ES>::T T;
    if (e.baseCell < 0) return;
    const uint32_t x = tid & (kMgrTile - 1), y0 = tid / kMgrTile;
    const int32_t cx = e.sCell[x];
    const int64_t ox = e.baseS + e.sOff[x];
    constexpr int kPer = kMgrTile * kMgrTile / kMgrThreads;
    // All of a lane's loads are issued before the first one is used, none under a branch.  A coordinate in the padding loads one of
    // the lane's own valid elements again (found first, from the edge table alone) — never anything else: only the cells the tile's
    // valid elements lie in are known to be mapped and ordered — and the store phase never looks at its tile word.
    if (cx < 0) return;
    int32_t cf = -1;
    int64_t of = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kPer; ++j) {
        const uint32_t y = y0 + (uint32_t)j * (kMgrThreads / kMgrTile);
        if (cf < 0 && e.sCell[kMgrTile + y] >= 0) { cf = e.sCell[kMgrTile + y]; of = e.sOff[kMgrTile + y]; }
    }
    if (cf < 0) return;
    T v[kPer];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kPer; ++j) {
        const uint32_t y = y0 + (uint32_t)j * (kMgrThreads / kMgrTile);
        const int32_t cy = e.sCell[kMgrTile + y];
        const bool ok = cy >= 0;
        v[j] = static_cast<const T*>(mgr_src(a, (uint32_t)(e.baseCell + cx + (ok ? cy : cf))))[ox + (ok ? e.sOff[kMgrTile + y] : of)];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kPer; ++j) tile[(y0 + (uint32_t)j * (kMgrThreads / kMgrTile)) * kMgrPitch + x] = v[j];
}

template <int ES>
MGR_HD void mgr_tile_store(const MgrArgs& a, uint32_t by, uint32_t tid, const MgrTileEdges& e, const typename MgrWord<ES>::L* tile) {
    typedef typename MgrWord<ES>::T T;
    if (e.baseCell < 0) return;
    const uint32_t y = tid & (kMgrTile - 1), x0 = tid / kMgrTile;
    if (e.sCell[kMgrTile + y] < 0) return;
    T* d = static_cast<T*>(mgr_dst(a, by)) + e.baseD + e.dOff[kMgrTile + y];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kMgrTile * kMgrTile / kMgrThreads; ++j) {
        const uint32_t x = x0 + (uint32_t)j * (kMgrThreads / kMgrTile);
        if (e.sCell[x] >= 0) d[e.dOff[x]] = (T)tile[y * kMgrPitch + x];
    }
}

// ---- launch geometry: fills units / lprLog2 / tiles / work / gridX from the modes, the form and the lane width in bytes -------------
MGR_HD uint64_t mgr_min_u64(uint64_t x, uint64_t y) { return x < y ? x : y; }

inline void mgr_finish_args(MgrArgs& a, int form, int es, int laneBytes) {
    uint64_t all = 1;
    for (int k = 0; k < a.nModes; ++k) all *= a.mode[k].dLocal;
    a.units = 0; a.lprLog2 = 0; a.tilesX = a.tilesY = 1;
    if (form == MGR_ROWS) {
        const uint32_t v = (uint32_t)(laneBytes / es);
        a.outer = all / a.mode[a.fast].dLocal;
        a.work = a.outer;
        a.units = (a.mode[a.fast].dLocal + v - 1) / v;
        while ((1u << a.lprLog2) < a.units && a.lprLog2 < 8) ++a.lprLog2;
        const uint64_t rowsPerWg = (uint64_t)kMgrThreads >> a.lprLog2;
        a.gridX = (uint32_t)mgr_min_u64((a.outer + rowsPerWg - 1) / rowsPerWg, 1u << 16);
    } else if (form == MGR_TILE) {
        a.tilesX = (a.mode[a.fastX].dLocal + kMgrTile - 1) / kMgrTile;
        a.tilesY = (a.mode[a.fast].dLocal + kMgrTile - 1) / kMgrTile;
        a.outer = all / a.mode[a.fast].dLocal / a.mode[a.fastX].dLocal;
        a.work = a.outer * a.tilesX * a.tilesY;
        a.gridX = (uint32_t)mgr_min_u64(a.work, 1u << 20);
    } else {
        a.outer = all;
        a.work = all;
        a.gridX = (uint32_t)mgr_min_u64((all + kMgrThreads - 1) / kMgrThreads, 1u << 16);
    }
    if (a.gridX == 0) a.gridX = 1;
}
