// mg_copy.cpp — cutensorMgCopy of libcutensorMg.so: descriptor, workspace, plan, call, description and host replay.
// =====================================================================================================================================
// cutensorMgCopy: dst[modesDst] = src[modesSrc] between two block-cyclic layouts (any block sizes, grids, ragged extents and
// strides on either side).  The contraction (mg_contraction_exec.cpp) does not use it: its scatter of staged C pieces is still the host loop of identity
// cutensorPermute plans.
//
// Every handle device fills the destination cells it owns with ONE copy launch on its caller's stream (mg_redistribute.hip; the
// index arithmetic is mg_redistribute_layout.h) — preceded, when the cell tables do not fit the kernel arguments, by the launches of
// the table writer ("tableLaunches" of the description).  Source cells are read where they are, so nothing is staged: plan creation
// enables the peer mapping of exactly the (destination device, source device) pairs the plan reads across, or refuses.  The form is
// a property of the two descriptors and so the same on every device:
//   flat    the layouts are identical and every byte of a cell is a valid element: mg_copy_cells on whole cells
//   rows    both sides have element stride 1 on the same label: lanes along it, 16-byte lanes when both block sizes and every other
//           stride are multiples of 16 bytes (decided here, per plan; a call whose cell pointers are not 16-byte aligned runs the
//           element-lane kernel of the same form instead)
//   tile    both sides have an element stride 1, on different labels: 64 x 64 tiles transposed through LDS
//   gather  a side without an element stride 1: one element per lane
// Cell tables (pointers) travel in the kernel arguments up to kMgrArgCells cells; beyond that they go through the device workspace.
//
// Owners: cell c of a tensor lives on HIP device devices[c]; the launch for a destination cell runs on the handle entry that lists
// that device — when the handle lists one device several times (logical devices: tests and measurements on one GPU), the k-th cell on
// that device, in cell order, belongs to the (k mod m)-th of the m entries.
//
// Ordering (the fork / join of cutensorMgContraction): every launch runs behind everything already enqueued on EVERY stream of the
// call, and every stream ends behind every launch — whichever stream produced a source cell (one of a device outside the handle
// included) or still reads a destination cell, the call is ordered against it.  The event calls stay linear in the device count:
// stream 0 is the hub.  Every other stream records a start event, the hub waits for them all and records "all started", which the
// launching streams wait for; after the launches the same in reverse ("all done").  A one-device handle needs no event at all.
// =====================================================================================================================================
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <new>
#include <set>
#include <string>

#include "mg_internal.hpp"
#include "mg_kernels.h"

using namespace ctamd_mg;

struct cutensorMgCopyDescriptor {
    MgTensor dst, src;
    std::vector<int32_t> mDst, mSrc;
    std::vector<int> perm;                  // position in the source of the destination's mode k
    std::vector<int> dstOwner, srcOwner;    // handle entry of every cell (-1: a source cell on a device outside the handle)
};
namespace {
struct MgCopyLaunch {
    int form = MGR_GATHER, lane = 0;
    std::vector<int> cells;                 // destination cells, by slot
    MgrArgs args;                           // everything but the pointer tables, for the plan's lane width
};
}  // namespace
struct cutensorMgCopyPlan {
    cutensorMgCopyDescriptor desc;
    std::vector<int32_t> devices;                         // the handle's device list (the plan outlives nothing of the handle's)
    bool haveDevice = false;
    int es = 0;
    std::vector<std::vector<MgCopyLaunch>> launches;      // per handle entry
    std::vector<int64_t> localBytes, remoteBytes, workspace;
    std::vector<int> tableLaunches;                       // per handle entry: launches of the table writer ahead of the copy kernel
    std::vector<std::vector<int>> readOwners;             // per handle entry g: the other entries whose source cells g's launch reads (a diagnostic)
    // created with the plan on a handle with devices, two or more entries: [g] start of stream g ([0]: "all started", on the hub),
    // [n + g] done of stream g ([n]: "all done")
    std::vector<hipEvent_t> events;
};

namespace {

void mg_log(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void mg_log(const char* fmt, ...) {
    if (ctamdLogLevel() <= 0) return;
    va_list ap;
    va_start(ap, fmt);
    std::fputs("[cutensor-amd] ", stderr);
    std::vfprintf(stderr, fmt, ap);
    std::fputc('\n', stderr);
    va_end(ap);
}

std::vector<int> copy_owners(const cutensorMgHandle* h, const MgTensor& t) {
    std::map<int32_t, std::vector<int>> entries;
    for (size_t g = 0; g < h->devices.size(); ++g) entries[h->devices[g]].push_back((int)g);
    std::map<int32_t, size_t> seen;
    std::vector<int> out((size_t)t.numCells, -1);
    for (int64_t c = 0; c < t.numCells; ++c) {
        const auto it = entries.find(t.devices[(size_t)c]);
        if (it != entries.end()) out[(size_t)c] = it->second[seen[it->first]++ % it->second.size()];
    }
    return out;
}

int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

// byte offsets of the three cell tables inside a device's workspace; returns the size (0: the tables fit the kernel arguments)
int64_t copy_tables(int64_t nSrc, int64_t nDst, int64_t off[3]) {
    off[0] = 0;
    off[1] = align256(8 * nSrc);
    off[2] = off[1] + align256(8 * nDst);
    if (nDst == 0 || (nSrc <= kMgrArgCells && nDst <= kMgrArgCells)) return 0;
    return off[2] + align256(4 * nDst);
}

void copy_workspace(const cutensorMgCopyDescriptor& d, size_t nDev, std::vector<int64_t>& out) {
    std::vector<int64_t> nDst(nDev, 0);
    for (int o : d.dstOwner) ++nDst[(size_t)o];
    out.assign(nDev, 0);
    int64_t off[3];
    for (size_t g = 0; g < nDev; ++g) out[g] = copy_tables(d.src.numCells, nDst[g], off);
}

const char* copy_form_name(int form) {
    switch (form) {
        case MGR_FLAT: return "flat";
        case MGR_ROWS: return "rows";
        case MGR_TILE: return "tile";
        default: return "gather";
    }
}

// the modes of `a` (destination order) and the form / lane width the two layouts admit
int copy_form(const cutensorMgCopyDescriptor& d, int es, int64_t mostCellsPerDevice, MgrArgs& a, int* lane) {
    const MgTensor& D = d.dst;
    const MgTensor& S = d.src;
    std::memset(&a, 0, sizeof(a));
    a.nModes = (int32_t)D.n;
    bool same = D.elemStride == S.elemStride && D.blockStride == S.blockStride && D.cellElems == S.cellElems, full = true;
    int64_t cellValid = 1;
    for (uint32_t k = 0; k < D.n; ++k) {
        const int j = d.perm[k];
        MgrMode& m = a.mode[k];
        m.extent = (uint32_t)D.extent[k];
        m.dBlock = (uint32_t)D.blockSize[k]; m.dCount = (uint32_t)D.deviceCount[k]; m.dCellStride = (uint32_t)D.cellStride[k];
        m.dLocal = (uint32_t)(D.localBlocks[k] * D.blockSize[k]);
        m.sBlock = (uint32_t)S.blockSize[(size_t)j]; m.sCount = (uint32_t)S.deviceCount[(size_t)j]; m.sCellStride = (uint32_t)S.cellStride[(size_t)j];
        m.dElemStride = D.elemStride[k]; m.dBlockStride = D.blockStride[k];
        m.sElemStride = S.elemStride[(size_t)j]; m.sBlockStride = S.blockStride[(size_t)j];
        same = same && j == (int)k && m.dBlock == m.sBlock && m.dCount == m.sCount;
        full = full && D.extent[k] == (int64_t)m.dLocal * m.dCount;
        cellValid *= m.dLocal;
    }
    *lane = es;
    if (same && full && cellValid == D.cellElems && mostCellsPerDevice <= kMgCopyBatch) { *lane = 16; return MGR_FLAT; }
    // the stride-1 label of a side: packed layouts with leading blocks of one element have several modes of element stride 1 — the
    // one with the most local coordinates carries the lanes (ties: the first in that side's mode order)
    a.fast = a.fastX = -1;
    auto s_local = [&](int k) { const size_t j = (size_t)d.perm[(size_t)k]; return S.localBlocks[j] * S.blockSize[j]; };
    for (int k = 0; k < (int)D.n; ++k) {
        if (a.mode[k].dElemStride == 1 && (a.fast < 0 || a.mode[k].dLocal > a.mode[a.fast].dLocal)) a.fast = k;
        if (a.mode[k].sElemStride != 1) continue;
        if (a.fastX < 0 || s_local(k) > s_local(a.fastX) || (s_local(k) == s_local(a.fastX) && d.perm[(size_t)k] < d.perm[(size_t)a.fastX])) a.fastX = k;
    }
    // a label with element stride 1 on both sides beats two different ones: rows instead of a transposition
    if (a.fast >= 0 && a.fastX >= 0 && a.fast != a.fastX) {
        if (a.mode[a.fast].sElemStride == 1 && a.mode[a.fast].dLocal > 1) a.fastX = a.fast;
        else if (a.mode[a.fastX].dElemStride == 1 && a.mode[a.fastX].dLocal > 1) a.fast = a.fastX;
    }
    if (a.fast < 0 || a.fastX < 0) return MGR_GATHER;
    if (a.fast != a.fastX) return MGR_TILE;
    const int64_t v = 16 / es;
    bool wide = a.mode[a.fast].dBlock % v == 0 && a.mode[a.fast].sBlock % v == 0;
    for (int k = 0; k < (int)D.n && wide; ++k) {
        const MgrMode& m = a.mode[k];
        if (k != a.fast && (m.dElemStride % v != 0 || m.sElemStride % v != 0)) wide = false;
        if (D.localBlocks[(size_t)k] > 1 && m.dBlockStride % v != 0) wide = false;
        if (S.localBlocks[(size_t)d.perm[(size_t)k]] > 1 && m.sBlockStride % v != 0) wide = false;
    }
    if (wide) *lane = 16;
    return MGR_ROWS;
}

// 16-byte lanes need 16-byte aligned cell buffers
bool copy_aligned16(const void* const* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if ((reinterpret_cast<uintptr_t>(p[i]) & 15u) != 0) return false;
    return true;
}

// The argument block of one launch for one call: the plan's, with the cell tables — inline, or (useW) as the three arrays `words`
// holds at off[], which the caller has made (or will make) readable at `tables`.  A 16-byte-lane plan falls back to element lanes
// for a call whose cell buffers are not 16-byte aligned.  Shared by the device path and the host replay.
MgrArgs copy_call_args(const cutensorMgCopyPlan& pl, const MgCopyLaunch& L, void* const* dst, const void* const* src, bool useW,
                       std::vector<uint64_t>& words, int64_t off[3], const char* tables, int* lane) {
    MgrArgs a = L.args;
    const size_t nSrc = (size_t)pl.desc.src.numCells, nDst = L.cells.size();
    std::vector<void*> dcells(nDst);
    for (size_t i = 0; i < nDst; ++i) dcells[i] = dst[L.cells[i]];
    *lane = L.lane;
    if (L.lane == 16 && !(copy_aligned16(src, nSrc) && copy_aligned16(dcells.data(), nDst))) {
        *lane = pl.es;
        mgr_finish_args(a, L.form, pl.es, *lane);
    }
    if (useW) {
        const int64_t bytes = copy_tables((int64_t)nSrc, (int64_t)nDst, off);
        words.assign((size_t)bytes / 8, 0);
        for (size_t c = 0; c < nSrc; ++c) words[c] = (uint64_t)reinterpret_cast<uintptr_t>(src[c]);
        for (size_t i = 0; i < nDst; ++i) words[(size_t)off[1] / 8 + i] = (uint64_t)reinterpret_cast<uintptr_t>(dcells[i]);
        int32_t* dc = reinterpret_cast<int32_t*>(words.data() + (size_t)off[2] / 8);
        for (size_t i = 0; i < nDst; ++i) dc[i] = (int32_t)L.cells[i];
        a.srcW = reinterpret_cast<const void* const*>(tables + off[0]);
        a.dstW = reinterpret_cast<void* const*>(tables + off[1]);
        a.dcellW = reinterpret_cast<const int32_t*>(tables + off[2]);
    } else {
        for (size_t c = 0; c < nSrc; ++c) a.src[c] = src[c];
        for (size_t i = 0; i < nDst; ++i) { a.dst[i] = dcells[i]; a.dcell[i] = (int32_t)L.cells[i]; }
    }
    return a;
}

// one launch over host memory, thread by thread
template <int ES>
void copy_replay_launch(const MgrArgs& a, int form, int lane) {
    for (uint32_t by = 0; by < (uint32_t)a.nCells; ++by)
        for (uint32_t bx = 0; bx < a.gridX; ++bx) {
            if (form == MGR_TILE) {
                std::vector<typename MgrWord<ES>::L> tile((size_t)kMgrTile * kMgrPitch);
                MgrTileEdges edges;
                for (uint64_t t = bx; t < a.work; t += a.gridX) {
                    for (uint32_t tid = 0; tid < (uint32_t)kMgrThreads; ++tid) mgr_tile_edges(a, by, t, tid, edges);
                    for (uint32_t tid = 0; tid < (uint32_t)kMgrThreads; ++tid) mgr_tile_load<ES>(a, tid, edges, tile.data());
                    for (uint32_t tid = 0; tid < (uint32_t)kMgrThreads; ++tid) mgr_tile_store<ES>(a, by, tid, edges, tile.data());
                }
                continue;
            }
            for (uint32_t tid = 0; tid < (uint32_t)kMgrThreads; ++tid) {
                if (form == MGR_GATHER) mgr_gather_thread<ES>(a, bx, by, tid);
                else if (lane == 16) mgr_rows_thread<ES, 16 / ES>(a, bx, by, tid);
                else mgr_rows_thread<ES, 1>(a, bx, by, tid);
            }
        }
}

}  // namespace

extern "C" {

// ---- the copy half of cuTENSORMg's public API (include/cutensorMg.h) ----------------------------------------------------------------
cutensorStatus_t cutensorMgCreateCopyDescriptor(const cutensorMgHandle_t handle, cutensorMgCopyDescriptor_t* desc,
                                                const cutensorMgTensorDescriptor_t descDst, const int32_t modesDst[],
                                                const cutensorMgTensorDescriptor_t descSrc, const int32_t modesSrc[]) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || descDst == nullptr || descSrc == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    const MgTensor& D = descDst->t;
    const MgTensor& S = descSrc->t;
    if ((D.n > 0 && modesDst == nullptr) || (S.n > 0 && modesSrc == nullptr)) return CUTENSOR_STATUS_INVALID_VALUE;
#define MG_REFUSE(STATUS, ...) do { mg_log("cutensorMgCreateCopyDescriptor: " __VA_ARGS__); return STATUS; } while (0)
    if (D.n > (uint32_t)kMgrMaxModes || S.n > (uint32_t)kMgrMaxModes)
        MG_REFUSE(CUTENSOR_STATUS_NOT_SUPPORTED, "%u / %u modes, more than the cap of %d", D.n, S.n, kMgrMaxModes);
    cutensorMgCopyDescriptor d;
    d.dst = D; d.src = S;
    d.mDst.assign(modesDst, modesDst + D.n);
    d.mSrc.assign(modesSrc, modesSrc + S.n);
    for (const std::vector<int32_t>* m : {&d.mDst, &d.mSrc})
        for (size_t i = 0; i < m->size(); ++i)
            for (size_t j = 0; j < i; ++j)
                if ((*m)[i] == (*m)[j]) MG_REFUSE(CUTENSOR_STATUS_INVALID_VALUE, "label %d is repeated in the %s", (int)(*m)[i], m == &d.mDst ? "destination" : "source");
    if (D.n != S.n) MG_REFUSE(CUTENSOR_STATUS_INVALID_VALUE, "the label sets differ (%u and %u modes)", D.n, S.n);
    for (uint32_t k = 0; k < D.n; ++k) {
        const int j = find_label(d.mSrc, d.mDst[k]);
        if (j < 0) MG_REFUSE(CUTENSOR_STATUS_INVALID_VALUE, "the label sets differ (label %d is not in the source)", (int)d.mDst[k]);
        if (D.extent[k] != S.extent[(size_t)j])
            MG_REFUSE(CUTENSOR_STATUS_INVALID_VALUE, "the extent of label %d differs (%lld and %lld)", (int)d.mDst[k], (long long)D.extent[k], (long long)S.extent[(size_t)j]);
        d.perm.push_back(j);
    }
    if (D.dtype != S.dtype) MG_REFUSE(CUTENSOR_STATUS_NOT_SUPPORTED, "different data types (%d and %d)", (int)D.dtype, (int)S.dtype);
    for (const MgTensor* t : {&D, &S}) {
        for (uint32_t k = 0; k < t->n; ++k) {
            if (t->localBlocks[k] * t->blockSize[k] * t->deviceCount[k] >= (1ll << 31))
                MG_REFUSE(CUTENSOR_STATUS_NOT_SUPPORTED, "a padded extent of 2^31 or more");
            if (t->elemStride[k] <= 0 || t->blockStride[k] <= 0) MG_REFUSE(CUTENSOR_STATUS_NOT_SUPPORTED, "a stride that is not positive");
        }
        if (t->numCells >= 65536) MG_REFUSE(CUTENSOR_STATUS_NOT_SUPPORTED, "65536 cells or more");
    }
    d.dstOwner = copy_owners(handle, D);
    d.srcOwner = copy_owners(handle, S);
    for (size_t c = 0; c < d.dstOwner.size(); ++c)
        if (d.dstOwner[c] < 0)
            MG_REFUSE(CUTENSOR_STATUS_NOT_SUPPORTED, "destination cell %zu lives on device %d, which is not in the handle", c, (int)D.devices[c]);
#undef MG_REFUSE
    *desc = new cutensorMgCopyDescriptor(std::move(d));
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyCopyDescriptor(cutensorMgCopyDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgCopyGetWorkspace(const cutensorMgHandle_t handle, const cutensorMgCopyDescriptor_t desc,
                                            int64_t deviceWorkspaceSize[], int64_t* hostWorkspaceSize) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || deviceWorkspaceSize == nullptr || hostWorkspaceSize == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    std::vector<int64_t> ws;
    copy_workspace(*desc, handle->devices.size(), ws);
    std::copy(ws.begin(), ws.end(), deviceWorkspaceSize);
    *hostWorkspaceSize = 0;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgCreateCopyPlan(const cutensorMgHandle_t handle, cutensorMgCopyPlan_t* plan,
                                          const cutensorMgCopyDescriptor_t desc,
                                          const int64_t deviceWorkspaceSize[], int64_t hostWorkspaceSize) try {
    (void)hostWorkspaceSize;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || desc == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    const int nDev = (int)handle->devices.size();
    std::unique_ptr<cutensorMgCopyPlan> pl(new cutensorMgCopyPlan());
    pl->desc = *desc;
    pl->devices = handle->devices;
    pl->haveDevice = handle->haveDevice;
    const cutensorMgCopyDescriptor& d = pl->desc;
    pl->es = (int)elem_size(d.dst.dtype);
    copy_workspace(d, (size_t)nDev, pl->workspace);
    for (int g = 0; g < nDev; ++g)
        if (pl->workspace[(size_t)g] > 0 && (deviceWorkspaceSize == nullptr || deviceWorkspaceSize[g] < pl->workspace[(size_t)g])) {
            mg_log("cutensorMgCreateCopyPlan: device %d needs %lld bytes of workspace for its cell tables", g, (long long)pl->workspace[(size_t)g]);
            return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
        }
    // ---- launches: every destination cell of a device in one launch ----
    pl->launches.assign((size_t)nDev, {});
    std::vector<std::vector<int>> cellsOf((size_t)nDev);
    for (size_t c = 0; c < d.dstOwner.size(); ++c) cellsOf[(size_t)d.dstOwner[c]].push_back((int)c);
    int64_t most = 0;
    for (const std::vector<int>& v : cellsOf) most = std::max<int64_t>(most, (int64_t)v.size());
    MgrArgs base;
    int lane = 0;
    const int form = copy_form(d, pl->es, most, base, &lane);
    for (int g = 0; g < nDev; ++g) {
        if (cellsOf[(size_t)g].empty()) continue;
        MgCopyLaunch L;
        L.form = form; L.lane = lane; L.cells = cellsOf[(size_t)g];
        L.args = base;
        L.args.nCells = (int32_t)L.cells.size();
        if (form != MGR_FLAT) mgr_finish_args(L.args, form, pl->es, lane);
        pl->launches[(size_t)g].push_back(std::move(L));
    }
    // ---- who reads whom, and how many valid bytes.  The elements a (destination cell, source cell) pair shares are a product over
    // modes of the indices the two grid coordinates share; only pairs of coordinates that share some are walked (per mode: the
    // stretches between two block edges of either side), so the work is the number of cell pairs that really exchange data
    struct Share { uint32_t dc, sc; int64_t n; };
    std::vector<std::vector<Share>> share(d.dst.n);
    for (uint32_t k = 0; k < d.dst.n; ++k) {
        const MgrMode& m = base.mode[k];
        std::map<std::pair<uint32_t, uint32_t>, int64_t> cnt;
        for (uint64_t i = 0; i < m.extent;) {
            const uint64_t next = std::min<uint64_t>({(i / m.dBlock + 1) * m.dBlock, (i / m.sBlock + 1) * m.sBlock, (uint64_t)m.extent});
            cnt[{(uint32_t)((i / m.dBlock) % m.dCount), (uint32_t)((i / m.sBlock) % m.sCount)}] += (int64_t)(next - i);
            i = next;
        }
        for (const auto& c : cnt) share[k].push_back(Share{c.first.first, c.first.second, c.second});
    }
    pl->localBytes.assign((size_t)nDev, 0);
    pl->remoteBytes.assign((size_t)nDev, 0);
    pl->readOwners.assign((size_t)nDev, {});
    std::vector<std::set<int>> readers((size_t)nDev);
    std::set<std::pair<int32_t, int32_t>> peers;      // (destination device, source device) pairs on different devices
    const std::function<void(uint32_t, int64_t, int64_t, int64_t)> walk = [&](uint32_t k, int64_t cd, int64_t cs, int64_t n) {
        if (k < d.dst.n) {
            for (const Share& s : share[k]) walk(k + 1, cd + (int64_t)s.dc * base.mode[k].dCellStride, cs + (int64_t)s.sc * base.mode[k].sCellStride, n * s.n);
            return;
        }
        const int g = d.dstOwner[(size_t)cd], o = d.srcOwner[(size_t)cs];
        const bool local = d.dst.devices[(size_t)cd] == d.src.devices[(size_t)cs];
        (local ? pl->localBytes : pl->remoteBytes)[(size_t)g] += n * pl->es;
        if (!local) peers.insert({d.dst.devices[(size_t)cd], d.src.devices[(size_t)cs]});
        if (o >= 0 && o != g) readers[(size_t)g].insert(o);
    };
    walk(0, 0, 0, 1);
    for (int g = 0; g < nDev; ++g) pl->readOwners[(size_t)g].assign(readers[(size_t)g].begin(), readers[(size_t)g].end());
    pl->tableLaunches.assign((size_t)nDev, 0);
    for (int g = 0; g < nDev; ++g)
        if (pl->workspace[(size_t)g] > 0 && !pl->launches[(size_t)g].empty())
            pl->tableLaunches[(size_t)g] = (int)((pl->workspace[(size_t)g] / 8 + kMgrTableWords - 1) / kMgrTableWords);
    if (handle->haveDevice) {
        DeviceGuard guard;
        // Remote cells are read in place: every (destination device, source device) pair of THIS plan gets its peer mapping here — the
        // handle only maps its own devices onto each other, and a source cell may live outside the handle — or the plan is refused
        for (const auto& pr : peers) {
            int can = 0;
            bool ok = hipSetDevice(pr.first) == hipSuccess && hipDeviceCanAccessPeer(&can, pr.first, pr.second) == hipSuccess && can != 0;
            if (ok) {
                const hipError_t e = hipDeviceEnablePeerAccess(pr.second, 0);
                ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            }
            (void)hipGetLastError();
            if (!ok) {
                mg_log("cutensorMgCreateCopyPlan: device %d has no peer access to device %d, which owns source cells it reads", (int)pr.first, (int)pr.second);
                return CUTENSOR_STATUS_NOT_SUPPORTED;
            }
        }
        // the fork / join events: with the plan, so that a call changes nothing in it
        if (nDev > 1) {
            pl->events.assign((size_t)(2 * nDev), nullptr);
            for (int i = 0; i < 2 * nDev; ++i)
                if (hipSetDevice(handle->devices[(size_t)(i % nDev)]) != hipSuccess ||
                    hipEventCreateWithFlags(&pl->events[(size_t)i], hipEventDisableTiming) != hipSuccess) {
                    (void)hipGetLastError();
                    cutensorMgDestroyCopyPlan(pl.release());
                    return CUTENSOR_STATUS_INTERNAL_ERROR;
                }
        }
    }
    *plan = pl.release();
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyCopyPlan(cutensorMgCopyPlan_t plan) try {
    if (plan == nullptr) return CUTENSOR_STATUS_SUCCESS;
    if (!plan->events.empty()) {
        DeviceGuard guard;
        const size_t nDev = plan->devices.size();
        for (size_t i = 0; i < plan->events.size(); ++i) {
            if (plan->events[i] == nullptr) continue;
            (void)hipSetDevice(plan->devices[i % nDev]);
            (void)hipEventDestroy(plan->events[i]);
        }
    }
    delete plan;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgCopy(const cutensorMgHandle_t handle, const cutensorMgCopyPlan_t plan,
                                void* ptrDst[], const void* ptrSrc[],
                                void* deviceWorkspace[], void* hostWorkspace, cudaStream_t streams[]) try {
    (void)hostWorkspace;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || ptrDst == nullptr || ptrSrc == nullptr || streams == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (!handle->haveDevice) return CUTENSOR_STATUS_ARCH_MISMATCH;   // plan-only handle (no GPU visible)
    const cutensorMgCopyPlan* pl = plan;
    const cutensorMgCopyDescriptor& d = pl->desc;
    if (handle->devices != pl->devices || !pl->haveDevice) return CUTENSOR_STATUS_INVALID_VALUE;    // the plan belongs to another handle
    const int nDev = (int)pl->devices.size();
    for (int64_t c = 0; c < d.dst.numCells; ++c) if (ptrDst[c] == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    for (int64_t c = 0; c < d.src.numCells; ++c) if (ptrSrc[c] == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    for (int g = 0; g < nDev; ++g)      // the cell tables are arrays of pointers
        if (pl->workspace[(size_t)g] > 0 && (deviceWorkspace == nullptr || deviceWorkspace[g] == nullptr || (reinterpret_cast<uintptr_t>(deviceWorkspace[g]) & 7u) != 0))
            return CUTENSOR_STATUS_INVALID_VALUE;
    DeviceGuard guard;
#define MG_HIP(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return CUTENSOR_STATUS_EXECUTION_FAILED; } } while (0)
    auto ev = [&](int i) { return pl->events[(size_t)i]; };      // [g] start of stream g, [0] all started; [n + g] done, [n] all done
    // ---- fork: every launch goes behind everything enqueued on every stream; stream 0 is the hub ----
    if (nDev > 1) {
        for (int g = 1; g < nDev; ++g) {
            MG_HIP(hipSetDevice(pl->devices[(size_t)g]));
            MG_HIP(hipEventRecord(ev(g), streams[g]));
        }
        MG_HIP(hipSetDevice(pl->devices[0]));
        for (int g = 1; g < nDev; ++g) MG_HIP(hipStreamWaitEvent(streams[0], ev(g), 0));
        MG_HIP(hipEventRecord(ev(0), streams[0]));
    }
    // ---- one copy launch per destination device (behind its table writer, if any), on its caller's stream ----
    std::vector<uint64_t> words;
    for (int g = 0; g < nDev; ++g) {
        if (pl->launches[(size_t)g].empty()) continue;
        MG_HIP(hipSetDevice(pl->devices[(size_t)g]));
        if (g > 0) MG_HIP(hipStreamWaitEvent(streams[g], ev(0), 0));
        for (const MgCopyLaunch& L : pl->launches[(size_t)g]) {
            if (L.form == MGR_FLAT) {
                MgCopyBatch batch;
                for (int c : L.cells) {
                    batch.src[batch.n] = ptrSrc[c];
                    batch.dst[batch.n] = ptrDst[c];
                    batch.bytes[batch.n++] = (uint64_t)d.dst.cellElems * (uint64_t)pl->es;
                }
                MG_HIP(mg_copy_cells(batch, streams[g]));
                continue;
            }
            const bool useW = pl->workspace[(size_t)g] > 0;
            int64_t off[3];
            int lane = 0;
            const MgrArgs a = copy_call_args(*pl, L, ptrDst, ptrSrc, useW, words, off, useW ? static_cast<const char*>(deviceWorkspace[g]) : nullptr, &lane);
            if (useW) MG_HIP(mg_redistribute_table(deviceWorkspace[g], words.data(), words.size() * 8, streams[g]));
            MG_HIP(mg_redistribute(a, L.form, pl->es, lane, streams[g]));
        }
        if (g > 0) MG_HIP(hipEventRecord(ev(nDev + g), streams[g]));
    }
    // ---- join: every stream ends behind every launch ----
    if (nDev > 1) {
        MG_HIP(hipSetDevice(pl->devices[0]));
        for (int g = 1; g < nDev; ++g)
            if (!pl->launches[(size_t)g].empty()) MG_HIP(hipStreamWaitEvent(streams[0], ev(nDev + g), 0));
        MG_HIP(hipEventRecord(ev(nDev), streams[0]));
        for (int g = 1; g < nDev; ++g) {
            MG_HIP(hipSetDevice(pl->devices[(size_t)g]));
            MG_HIP(hipStreamWaitEvent(streams[g], ev(nDev), 0));
        }
    }
#undef MG_HIP
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// ---- diagnostics of the copy (not part of the cuTENSORMg ABI) ----------------------------------------------------------------------
// The plan as JSON: per handle entry its launches (form, lane width in bytes, destination cells, grid; the flat form sizes its own
// grid.x at launch, reported as 0), the valid bytes it reads from cells on its own device and from others, its workspace, the
// launches of the table writer that precede the copy kernel when the cell tables go through that workspace, and the entries it
// reads from; the owner of every cell, the mode cap and the number of cells the kernel arguments hold.
int ctamdMgDescribeCopyPlan(const cutensorMgCopyPlan_t plan, char* buf, size_t len) try {
    if (plan == nullptr || buf == nullptr || len == 0) return -1;
    std::string s;
    char tmp[256];
    auto add = [&](const char* fmt, auto... a) { std::snprintf(tmp, sizeof(tmp), fmt, a...); s += tmp; };
    auto list = [&](const char* name, const std::vector<int>& v) {
        add("\"%s\":[", name);
        for (size_t i = 0; i < v.size(); ++i) add("%s%d", i ? "," : "", v[i]);
        s += "]";
    };
    add("{\"modeCap\":%d,\"argCells\":%d,\"hostWorkspace\":0,\"elementSize\":%d,", kMgrMaxModes, kMgrArgCells, plan->es);
    list("dstOwners", plan->desc.dstOwner);
    s += ",";
    list("srcOwners", plan->desc.srcOwner);
    s += ",\"devices\":[";
    for (size_t g = 0; g < plan->launches.size(); ++g) {
        add("%s{\"dev\":%d,\"localBytes\":%lld,\"remoteBytes\":%lld,\"workspace\":%lld,\"tableLaunches\":%d,", g ? "," : "", (int)g, (long long)plan->localBytes[g],
            (long long)plan->remoteBytes[g], (long long)plan->workspace[g], plan->tableLaunches[g]);
        list("readOwners", plan->readOwners[g]);
        s += ",\"launches\":[";
        for (size_t i = 0; i < plan->launches[g].size(); ++i) {
            const MgCopyLaunch& L = plan->launches[g][i];
            add("%s{\"form\":\"%s\",\"lane\":%d,\"grid\":[%u,%d],", i ? "," : "", copy_form_name(L.form), L.lane, L.form == MGR_FLAT ? 0u : L.args.gridX, (int)L.cells.size());
            // the labels the lanes run along: the destination's, the source's (rows: the same one; flat / gather: -1)
            const bool along = L.form == MGR_ROWS || L.form == MGR_TILE;
            add("\"along\":[%d,%d],", along ? (int)plan->desc.mDst[(size_t)L.args.fast] : -1, along ? (int)plan->desc.mDst[(size_t)L.args.fastX] : -1);
            list("cells", L.cells);
            s += "}";
        }
        s += "]}";
    }
    s += "]}";
    if (s.size() + 1 > len) return -(int)(s.size() + 1);
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
} CTAMD_API_CATCH_INT

// Walks the plan's launch tables over HOST cell buffers: the same launches, cells, forms and argument blocks as cutensorMgCopy, every
// kernel executed thread by thread through the bodies of mg_redistribute_layout.h (the flat form is a copy of whole cells).  A
// 16-byte-lane plan is not quietly replayed with element lanes: cell buffers that are not 16-byte aligned are an error (-3).
// Returns 0, -1 for invalid arguments.
int ctamdMgCopyReplayOnHost(const cutensorMgCopyPlan_t plan, void* const dst[], const void* const src[]) try {
    if (plan == nullptr || dst == nullptr || src == nullptr) return -1;
    const cutensorMgCopyPlan& pl = *plan;
    for (int64_t c = 0; c < pl.desc.dst.numCells; ++c) if (dst[c] == nullptr) return -1;
    for (int64_t c = 0; c < pl.desc.src.numCells; ++c) if (src[c] == nullptr) return -1;
    for (size_t g = 0; g < pl.launches.size(); ++g)
        for (const MgCopyLaunch& L : pl.launches[g]) {
            if (L.form == MGR_FLAT) {
                for (int c : L.cells) std::memcpy(dst[c], src[c], (size_t)pl.desc.dst.cellElems * (size_t)pl.es);
                continue;
            }
            std::vector<uint64_t> words;
            int64_t off[3];
            int lane = 0;
            const bool useW = pl.workspace[g] > 0;
            MgrArgs a = copy_call_args(pl, L, dst, src, useW, words, off, nullptr, &lane);
            if (lane != L.lane) return -3;
            if (useW) {      // the tables are read where they were built
                const char* tables = reinterpret_cast<const char*>(words.data());
                a.srcW = reinterpret_cast<const void* const*>(tables + off[0]);
                a.dstW = reinterpret_cast<void* const*>(tables + off[1]);
                a.dcellW = reinterpret_cast<const int32_t*>(tables + off[2]);
            }
            switch (pl.es) {
                case 2: copy_replay_launch<2>(a, L.form, lane); break;
                case 4: copy_replay_launch<4>(a, L.form, lane); break;
                default: copy_replay_launch<8>(a, L.form, lane); break;
            }
        }
    return 0;
} CTAMD_API_CATCH_INT

}  // extern "C"
