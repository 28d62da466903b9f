// mp_geometry.h — the box arithmetic of cuTENSORMp: which part of a distributed tensor a rank owns, which part it needs, where a box
// starts inside a block, and how a strided copy of a box falls into modes and launches.  Integers only: no HIP call, no cutensor call
// (tests/harness/mp_geometry_harness.cpp checks it on the CPU against brute-force enumeration).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include <hip/library_types.h>   // hipDataType

// internal to libcutensorMp.so: the library exports its C entry points only
#define CTAMD_MP_HIDDEN __attribute__((visibility("hidden")))

namespace ctamd_mp CTAMD_MP_HIDDEN {

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct MpTensor {
    uint32_t n = 0;
    hipDataType dtype = HIP_R_32F;
    std::vector<int64_t> extent, p, bs, elemStride, cellStride;
    int64_t numCells = 1;
    std::vector<int32_t> owner;     // rank of each cell; empty = replicated on every rank
    bool packed = true;             // elemStride is the packed layout over bs
    bool replicated() const { return owner.empty(); }
};

struct Box {
    std::vector<int64_t> lo, hi;
    bool empty() const {
        for (size_t i = 0; i < lo.size(); ++i) if (hi[i] <= lo[i]) return true;
        return false;
    }
    int64_t volume() const {
        int64_t v = 1;
        for (size_t i = 0; i < lo.size(); ++i) v *= std::max<int64_t>(0, hi[i] - lo[i]);
        return v;
    }
    bool operator==(const Box& o) const { return lo == o.lo && hi == o.hi; }
};

inline Box cell_box(const MpTensor& t, int64_t cell) {
    Box b; b.lo.resize(t.n); b.hi.resize(t.n);
    for (uint32_t i = 0; i < t.n; ++i) {
        const int64_t c = t.replicated() ? 0 : (cell / t.cellStride[i]) % t.p[i];
        b.lo[i] = c * t.bs[i];
        b.hi[i] = std::min(t.extent[i], b.lo[i] + t.bs[i]);
    }
    return b;
}
inline Box whole_box(const std::vector<int64_t>& extent) {
    Box b; b.lo.assign(extent.size(), 0); b.hi = extent;
    return b;
}
inline Box intersect(const Box& a, const Box& b) {
    Box r; r.lo.resize(a.lo.size()); r.hi.resize(a.lo.size());
    for (size_t i = 0; i < a.lo.size(); ++i) { r.lo[i] = std::max(a.lo[i], b.lo[i]); r.hi[i] = std::min(a.hi[i], b.hi[i]); }
    return r;
}
inline int64_t cell_of_rank(const MpTensor& t, int rank) {
    if (t.replicated()) return 0;
    for (int64_t c = 0; c < t.numCells; ++c) if (t.owner[c] == rank) return c;
    return -1;
}
inline Box block_of_rank(const MpTensor& t, int rank) { return cell_box(t, cell_of_rank(t, rank)); }
inline int find_label(const std::vector<int32_t>& v, int32_t l) {
    for (size_t i = 0; i < v.size(); ++i) if (v[i] == l) return (int)i;
    return -1;
}

// The box of operand x (modes mx) a rank needs to compute the box cBox of C (modes mC): C's range in the modes they share, the full
// extent in the others.
inline Box needed_box(const MpTensor& x, const std::vector<int32_t>& mx, const std::vector<int32_t>& mC, const Box& cBox) {
    Box b; b.lo.resize(x.n); b.hi.resize(x.n);
    for (uint32_t i = 0; i < x.n; ++i) {
        const int j = find_label(mC, mx[i]);
        if (j >= 0) { b.lo[i] = cBox.lo[j]; b.hi[i] = cBox.hi[j]; }
        else { b.lo[i] = 0; b.hi[i] = x.extent[i]; }
    }
    return b;
}

inline std::vector<int64_t> packed_strides(const std::vector<int64_t>& ext) {
    std::vector<int64_t> s(ext.size());
    int64_t run = 1;
    for (size_t i = 0; i < ext.size(); ++i) { s[i] = run; run *= ext[i]; }
    return s;
}
inline std::vector<int64_t> sizes(const Box& b) {
    std::vector<int64_t> s(b.lo.size());
    for (size_t i = 0; i < s.size(); ++i) s[i] = b.hi[i] - b.lo[i];
    return s;
}
// element offset of box b's first element in a tensor of strides `stride` whose element 0 is origin's first
inline int64_t box_offset(const Box& b, const Box& origin, const std::vector<int64_t>& stride) {
    int64_t off = 0;
    for (size_t i = 0; i < b.lo.size(); ++i) off += (b.lo[i] - origin.lo[i]) * stride[i];
    return off;
}
// a box that is one contiguous run of a packed tensor of extents `full`
inline bool contiguous_in(const Box& b, const std::vector<int64_t>& full) {
    bool partialSeen = false;
    for (size_t i = 0; i < full.size(); ++i) {
        const int64_t sz = b.hi[i] - b.lo[i];
        if (partialSeen && sz != 1) return false;
        if (sz != full[i]) partialSeen = true;
    }
    return true;
}
inline uint32_t alignment_of(int64_t byteOffset) {       // largest power of two <= 256 dividing the offset
    uint32_t a = 256;
    while (a > 1 && (byteOffset % a) != 0) a >>= 1;
    return a;
}

// ---- the modes and launches of a strided copy --------------------------------------------------------------------
struct CMode { int64_t extent, sSrc, sDst; };
using Launches = std::vector<std::pair<int64_t, int64_t>>;   // (src, dst) element offsets added to the base pointers

// modes of a copy: box `b` read at `srcStride`, written at `dstStride`
inline std::vector<CMode> copy_modes(const Box& b, const std::vector<int64_t>& srcStride, const std::vector<int64_t>& dstStride) {
    std::vector<CMode> m;
    for (size_t i = 0; i < b.lo.size(); ++i) m.push_back(CMode{b.hi[i] - b.lo[i], srcStride[i], dstStride[i]});
    return m;
}
// drop unit modes, fuse modes that are contiguous in both tensors
inline std::vector<CMode> fuse_modes(const std::vector<CMode>& modes) {
    std::vector<CMode> g;
    for (const CMode& m : modes) {
        if (m.extent == 1) continue;
        if (!g.empty() && m.sSrc == g.back().sSrc * g.back().extent && m.sDst == g.back().sDst * g.back().extent) { g.back().extent *= m.extent; continue; }
        g.push_back(m);
    }
    return g;
}
// Takes the smallest mode out of the view `g` and into the host loop: every launch becomes `extent` launches.  False when that would
// make more than kMaxCopyLaunches of them (g and launches are then unchanged).
constexpr int64_t kMaxCopyLaunches = 4096;
inline bool peel_smallest_mode(std::vector<CMode>& g, Launches& launches) {
    size_t k = 0;
    for (size_t i = 1; i < g.size(); ++i) if (g[i].extent < g[k].extent) k = i;
    const CMode m = g[k];
    if ((int64_t)launches.size() * m.extent > kMaxCopyLaunches) return false;
    g.erase(g.begin() + (long)k);
    Launches nl;
    for (const auto& l : launches)
        for (int64_t j = 0; j < m.extent; ++j) nl.push_back(std::make_pair(l.first + j * m.sSrc, l.second + j * m.sDst));
    launches.swap(nl);
    return true;
}
// Largest power of two <= 256 dividing every byte offset: what the copy may promise about its pointers (the bases it is added to —
// hipMalloc'ed user blocks, 256-byte-aligned workspace regions — are 256-byte aligned).
inline uint32_t common_alignment(const Launches& launches, bool second, int64_t es) {
    uint32_t a = 256;
    for (const auto& l : launches) {
        const int64_t bytes = (second ? l.second : l.first) * es;
        while (a > 1 && (bytes % a) != 0) a >>= 1;
    }
    return std::max<uint32_t>(a, (uint32_t)std::min<int64_t>(es, 16));
}

}  // namespace ctamd_mp
