// mg_views.cpp — the index arithmetic of libcutensorMg.so's local views: boxes of a ragged contracted mode, grid / local digits of a
// block index, the strided view of a tensor for a piece, the grid cells a view touches.  No HIP call.
#include <algorithm>

#include "mg_internal.hpp"

namespace ctamd_mg {

// Boxes that tile the valid part [0, extent) of a label's padded index space idx = w + blockSize * b,
// b = sum_j digit_j * prod_{i<j} f_i: the full blocks b < extent / blockSize as a mixed-radix prefix (one box per non-zero
// digit of the bound, most significant first), then the partial last block.  At most digits + 1 boxes; one box (everything)
// when the extent fills the padded space.
std::vector<Clip> kbox_list(int li, const Radix& r, int64_t extent) {
    std::vector<Clip> out;
    const int n = (int)r.f.size();
    const int64_t full = extent / r.blockSize, rem = extent % r.blockSize;
    auto all_digits = [&]() { std::vector<std::pair<int64_t, int64_t>> d((size_t)n); for (int j = 0; j < n; ++j) d[(size_t)j] = {0, r.f[(size_t)j]}; return d; };
    if (rem == 0 && full >= r.numBlocks) {
        Clip c; c.label = li; c.wHi = r.blockSize; c.digit = all_digits();
        out.push_back(c);
        return out;
    }
    std::vector<int64_t> below((size_t)n + 1, 1);
    for (int j = 0; j < n; ++j) below[(size_t)j + 1] = below[(size_t)j] * r.f[(size_t)j];
    // full blocks: b in [0, full)
    if (n == 0) {
        if (full >= 1) { Clip c; c.label = li; c.wHi = r.blockSize; out.push_back(c); }
    } else {
        std::vector<std::pair<int64_t, int64_t>> pinned = all_digits();
        for (int j = n - 1; j >= 0; --j) {
            const int64_t t = (full / below[(size_t)j]) % r.f[(size_t)j];
            const bool topOverflow = (j == n - 1) && full >= below[(size_t)n];   // bound beyond the padded space: cannot happen (full < numBlocks here)
            if (t > 0 && !topOverflow) {
                Clip c; c.label = li; c.wHi = r.blockSize; c.digit = pinned;
                c.digit[(size_t)j] = {0, t};
                for (int i = 0; i < j; ++i) c.digit[(size_t)i] = {0, r.f[(size_t)i]};
                out.push_back(c);
            }
            pinned[(size_t)j] = {t, t + 1};
        }
    }
    if (rem > 0) {   // the partial block b == full
        Clip c; c.label = li; c.wHi = rem; c.digit.resize((size_t)n);
        for (int j = 0; j < n; ++j) { const int64_t t = (full / below[(size_t)j]) % r.f[(size_t)j]; c.digit[(size_t)j] = {t, t + 1}; }
        out.push_back(c);
    }
    return out;
}

// digits of tensor t's mode i below `split` are grid-coordinate digits, the rest local-block digits
int grid_digits(const Radix& r, int64_t dc) {
    int64_t prod = 1;
    int k = 0;
    while (prod < dc && k < (int)r.f.size()) prod *= r.f[k++];
    return k;
}

// View of tensor T for a piece.  staging: strides of the [cell][cell buffer] image (grid digits step by whole cell
// images); otherwise the view is relative to one cell buffer and grid digits must be pinned (they contribute no offset).
View make_view(const MgTensor& t, const std::vector<int32_t>& labels, const std::vector<int32_t>& universe,
               const std::vector<Radix>& radix, const Restrict& rs, bool staging) {
    View v;
    for (uint32_t i = 0; i < t.n; ++i) {
        const int li = find_label(universe, labels[i]);
        const Radix& r = radix[li];
        const int nGrid = grid_digits(r, t.deviceCount[i]);
        const bool isP = rs.is_p(li), isQ = li == rs.qLabel;
        const int64_t pLo = isP ? rs.plo(li) : 0, pHi = isP ? rs.phi(li) : 0;
        const Clip* clip = rs.clip_of(li);
        // w: position inside a block
        if (clip != nullptr) {
            if (clip->wHi > 1) { v.extent.push_back(clip->wHi); v.stride.push_back(t.elemStride[i]); v.modes.push_back(8 * li + 7); }
        } else if (isP) {
            const int64_t block = pLo / r.blockSize;
            v.offset += (pLo - block * r.blockSize) * t.elemStride[i];
            if (pHi - pLo > 1) { v.extent.push_back(pHi - pLo); v.stride.push_back(t.elemStride[i]); v.modes.push_back(8 * li + 7); }
        } else if (r.blockSize > 1) {
            v.extent.push_back(r.blockSize); v.stride.push_back(t.elemStride[i]); v.modes.push_back(8 * li + 7);
        }
        // block-index digits
        int64_t rest = isP ? pLo / r.blockSize : 0;
        int64_t gridStep = t.cellElems * t.cellStride[i], localStep = t.blockStride[i];
        for (int j = 0; j < (int)r.f.size(); ++j) {
            const bool grid = j < nGrid;
            const int64_t step = grid ? gridStep : localStep;
            if (grid && !staging) {           // cell-relative view: the cell is chosen by the caller, its coordinate is no mode
                if (isP) rest /= r.f[j];
                gridStep *= r.f[j];
                continue;
            }
            if (clip != nullptr) {
                const int64_t lo = clip->digit[(size_t)j].first, hi = clip->digit[(size_t)j].second;
                v.offset += lo * step;
                if (hi - lo > 1) { v.extent.push_back(hi - lo); v.stride.push_back(step); v.modes.push_back(8 * li + j); }
            } else if (isP) {
                v.offset += (rest % r.f[j]) * step;
                rest /= r.f[j];
            } else if (isQ && j == rs.qDigit) {
                v.offset += rs.c0 * step;
                if (rs.c1 - rs.c0 > 1) { v.extent.push_back(rs.c1 - rs.c0); v.stride.push_back(step); v.modes.push_back(8 * li + j); }
            } else if (r.f[j] > 1) {
                v.extent.push_back(r.f[j]); v.stride.push_back(step); v.modes.push_back(8 * li + j);
            }
            if (grid) gridStep *= r.f[j]; else localStep *= r.f[j];
        }
    }
    return v;
}

// Grid cells of tensor T the restricted view touches.
std::vector<int> cells_of(const MgTensor& t, const std::vector<int32_t>& labels, const std::vector<int32_t>& universe,
                          const std::vector<Radix>& radix, const Restrict& rs) {
    std::vector<int> out;
    for (int64_t c = 0; c < t.numCells; ++c) {
        bool want = true;
        for (uint32_t i = 0; i < t.n && want; ++i) {
            const int li = find_label(universe, labels[i]);
            const int64_t coord = (c / t.cellStride[i]) % t.deviceCount[i];
            if (rs.is_p(li)) {
                want = coord == (rs.plo(li) / radix[li].blockSize) % t.deviceCount[i];
            } else if (li == rs.qLabel && rs.qDigit >= 0 && rs.qDigit < grid_digits(radix[li], t.deviceCount[i])) {
                // q's cut digit is a grid digit of this tensor: its value inside the cell coordinate
                int64_t below = 1;
                for (int j = 0; j < rs.qDigit; ++j) below *= radix[li].f[j];
                const int64_t d = (coord / below) % radix[li].f[rs.qDigit];
                want = d >= rs.c0 && d < rs.c1;
            }
        }
        if (want) out.push_back((int)c);
    }
    return out;
}

uint32_t align_of(int64_t offsetBytes, size_t es) {   // pointer alignment a view at this byte offset of a 256-byte aligned base keeps
    uint32_t a = 256;
    while (a > es && (offsetBytes % a) != 0) a >>= 1;
    return std::max<uint32_t>(a, (uint32_t)es);
}

}  // namespace ctamd_mg
