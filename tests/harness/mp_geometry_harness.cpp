// mp_geometry_harness.cpp — the box arithmetic of libcutensorMp.so (csrc/mp/mp_geometry.h) on its own, on the CPU, against brute-force
// enumeration of every element on extents <= 7: cell_box on ragged and empty cells, intersect, needed_box, contiguous_in, box_offset,
// and the fusion / peeling of a copy's modes (the launch offsets together with the remaining view must visit exactly the elements of
// the box, each once, at the right place in both tensors).  Stand-alone: no HIP runtime, no libcutensor.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

#include "../../cudalibrarysamples_amd/csrc/mp/mp_geometry.h"

using namespace ctamd_mp;

static int g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static MpTensor tensor(const std::vector<int64_t>& extent, const std::vector<int64_t>& p, const std::vector<int64_t>& bs = {}) {
    MpTensor t;
    t.n = (uint32_t)extent.size();
    t.extent = extent; t.p = p;
    t.bs.resize(t.n); t.cellStride.resize(t.n);
    int64_t cells = 1;
    for (uint32_t i = 0; i < t.n; ++i) {
        t.bs[i] = bs.empty() ? (extent[i] + p[i] - 1) / p[i] : bs[i];
        t.cellStride[i] = cells;
        cells *= p[i];
    }
    t.elemStride = packed_strides(t.bs);
    t.numCells = cells;
    if (cells > 1) for (int64_t c = 0; c < cells; ++c) t.owner.push_back((int32_t)(cells - 1 - c));   // ranks in reverse cell order
    return t;
}

// every index tuple of a box, first mode fastest
static std::vector<std::vector<int64_t>> elements(const Box& b) {
    std::vector<std::vector<int64_t>> out;
    if (b.empty()) return out;
    std::vector<int64_t> idx = b.lo;
    for (;;) {
        out.push_back(idx);
        size_t i = 0;
        while (i < idx.size() && ++idx[i] == b.hi[i]) { idx[i] = b.lo[i]; ++i; }
        if (i == idx.size()) return out;
    }
}
static bool inside(const Box& b, const std::vector<int64_t>& idx) {
    for (size_t i = 0; i < idx.size(); ++i) if (idx[i] < b.lo[i] || idx[i] >= b.hi[i]) return false;
    return true;
}

// cells tile the tensor: every element lies in exactly one cell; ragged last cells are cut at the extent, cells beyond it are empty
static void check_cells(const MpTensor& t) {
    const Box whole = whole_box(t.extent);
    int64_t volume = 0;
    for (int64_t c = 0; c < t.numCells; ++c) {
        const Box b = cell_box(t, c);
        CHECK(b.empty() == (elements(b).size() == 0));
        CHECK(b.volume() == (int64_t)elements(b).size());
        volume += b.volume();
        for (const auto& e : elements(b)) CHECK(inside(whole, e));
        if (!t.replicated()) CHECK(cell_of_rank(t, t.owner[(size_t)c]) == c);
    }
    CHECK(volume == whole.volume());
    for (const auto& e : elements(whole)) {
        int owners = 0;
        for (int64_t c = 0; c < t.numCells; ++c) owners += inside(cell_box(t, c), e) ? 1 : 0;
        CHECK(owners == 1);
    }
}

static void check_intersect(const Box& a, const Box& b, const Box& whole) {
    const Box r = intersect(a, b);
    int64_t n = 0;
    for (const auto& e : elements(whole)) {
        const bool both = inside(a, e) && inside(b, e);
        CHECK(both == (!r.empty() && inside(r, e)));
        n += both ? 1 : 0;
    }
    CHECK(r.volume() == n || (r.empty() && n == 0));
}

// box_offset and contiguous_in against the linear index of every element of a packed tensor
static void check_offsets(const Box& b, const std::vector<int64_t>& full) {
    if (b.empty()) return;
    const std::vector<int64_t> stride = packed_strides(full);
    const Box whole = whole_box(full);
    std::set<int64_t> at;
    for (const auto& e : elements(b)) {
        int64_t lin = 0;
        for (size_t i = 0; i < e.size(); ++i) lin += e[i] * stride[i];
        at.insert(lin);
    }
    CHECK(*at.begin() == box_offset(b, whole, stride));
    const bool run = *at.rbegin() - *at.begin() + 1 == (int64_t)at.size();
    CHECK(run == contiguous_in(b, full));
}

// the copy of box `part` of a block laid out at `srcStride` into a tensor at `dstStride`: fused modes, then peeled `peels` times —
// launches x remaining view must map every element's source offset to its destination offset, each exactly once
static void check_copy(const Box& part, const Box& srcOrigin, const std::vector<int64_t>& srcStride, const Box& dstOrigin,
                       const std::vector<int64_t>& dstStride, int peels) {
    if (part.empty()) return;
    std::map<int64_t, int64_t> want;
    for (const auto& e : elements(part)) {
        int64_t s = 0, d = 0;
        for (size_t i = 0; i < e.size(); ++i) { s += (e[i] - srcOrigin.lo[i]) * srcStride[i]; d += (e[i] - dstOrigin.lo[i]) * dstStride[i]; }
        want[s] = d;
    }
    std::vector<CMode> g = fuse_modes(copy_modes(part, srcStride, dstStride));
    Launches launches(1, std::make_pair(box_offset(part, srcOrigin, srcStride), box_offset(part, dstOrigin, dstStride)));
    for (int i = 0; i < peels && !g.empty(); ++i) CHECK(peel_smallest_mode(g, launches));
    for (const CMode& m : g) CHECK(m.extent > 1);
    std::map<int64_t, int64_t> got;
    Box view; view.lo.assign(g.size(), 0);
    for (const CMode& m : g) view.hi.push_back(m.extent);
    std::vector<std::vector<int64_t>> idx = elements(view);
    if (g.empty()) idx.assign(1, std::vector<int64_t>());
    for (const auto& l : launches)
        for (const auto& e : idx) {
            int64_t s = l.first, d = l.second;
            for (size_t i = 0; i < e.size(); ++i) { s += e[i] * g[i].sSrc; d += e[i] * g[i].sDst; }
            CHECK(got.count(s) == 0);
            got[s] = d;
        }
    CHECK(got == want);
    CHECK(common_alignment(launches, false, 4) >= 4 && common_alignment(launches, true, 4) >= 4);
    for (const auto& l : launches) CHECK((l.first * 4) % common_alignment(launches, false, 4) == 0 && (l.second * 4) % common_alignment(launches, true, 4) == 0);
}

int main() {
    // ragged (7 over 2 and 3: blocks 4 and 3), empty cells (5 over 4: blocks of 2, the fourth cell starts at 6 > 5), replicated, oversized blocks
    const MpTensor tensors[] = {tensor({7, 5}, {2, 2}), tensor({7, 6, 3}, {3, 1, 2}), tensor({5, 3}, {4, 1}), tensor({3, 7}, {1, 1}),
                                tensor({4, 4, 3}, {1, 2, 1}, {5, 2, 4}), tensor({2, 2, 2, 2}, {2, 1, 2, 1})};
    for (const MpTensor& t : tensors) {
        check_cells(t);
        const Box whole = whole_box(t.extent);
        for (int64_t a = 0; a < t.numCells; ++a) {
            const Box ca = cell_box(t, a);
            check_offsets(ca, t.extent);
            // an arbitrary window of the tensor against every cell
            Box w = whole;
            for (uint32_t i = 0; i < t.n; ++i) { w.lo[i] = std::min<int64_t>(1, t.extent[i] - 1); w.hi[i] = std::max(w.lo[i] + 1, t.extent[i] - (int64_t)(i % 2)); }
            check_intersect(ca, w, whole);
            check_offsets(intersect(ca, w), t.extent);
            for (int64_t b = 0; b < t.numCells; ++b) check_intersect(ca, cell_box(t, b), whole);
            // the part of the window in this cell, copied from the cell's block into a packed tensor of the window — as a pack / unpack does
            const Box part = intersect(ca, w);
            for (int peels = 0; peels < 3; ++peels) {
                check_copy(part, ca, t.elemStride, w, packed_strides(sizes(w)), peels);
                check_copy(part, part, packed_strides(sizes(part)), ca, t.elemStride, peels);
            }
        }
    }
    // the empty fourth cell of 5 over 4
    CHECK(cell_box(tensors[2], 3).empty() && cell_box(tensors[2], 3).volume() == 0 && !cell_box(tensors[2], 2).empty());

    // needed_box: C[m, n] = A[m, k] B[k, n]; C's box fixes m of A and n of B, k is taken whole
    const MpTensor A = tensor({7, 6}, {1, 2}), B = tensor({6, 5}, {2, 1}), C = tensor({7, 5}, {2, 2});
    const std::vector<int32_t> mA = {'m', 'k'}, mB = {'k', 'n'}, mC = {'m', 'n'};
    for (int64_t c = 0; c < C.numCells; ++c) {
        const Box cb = cell_box(C, c);
        const Box na = needed_box(A, mA, mC, cb), nb = needed_box(B, mB, mC, cb);
        for (const auto& e : elements(whole_box(A.extent))) CHECK(inside(na, e) == (e[0] >= cb.lo[0] && e[0] < cb.hi[0]));
        for (const auto& e : elements(whole_box(B.extent))) CHECK(inside(nb, e) == (e[1] >= cb.lo[1] && e[1] < cb.hi[1]));
    }
    // a launch count beyond the limit is refused and leaves the view alone
    std::vector<CMode> g = {{4096, 1, 2}, {5000, 9000, 10000}};
    Launches many(2, std::make_pair<int64_t, int64_t>(0, 0));
    CHECK(!peel_smallest_mode(g, many) && g.size() == 2 && many.size() == 2);
    CHECK(alignment_of(0) == 256 && alignment_of(384) == 128 && alignment_of(12) == 4 && round_up(257, 256) == 512);
    std::printf("mp geometry ok: %d checks\n", g_checks);
    return 0;
}
