// mg.cpp — cuTENSORMg on a node of MI355X GPUs: single process, one host thread, N devices.
//
// Serves the call sequence of cuTENSORMg/contraction_multi_gpu.cu (create handle :151, block-cyclic
// tensor descriptors :195-217, contraction descriptor / find / workspace / plan :228-250,
// cutensorMgContraction :328-332) and of cuTENSORMg/blog_post.cu (:131-145, :286-302).  Built entirely
// on the public single-GPU ABI (include/cutensor.h), HIP and RCCL.
//
// Algorithm ("shard the largest free mode, gather the rest, overlap the gather with the first pieces"):
//   1. The largest free mode p of C (carried by exactly one operand X) is cut into one contiguous shard
//      per handle device; shards are cut again at p's block boundaries so that every piece lies in one block.
//   2. The other operand Y does not carry p: every device needs all of it (an all-gather).  When Y is
//      distributed along a free mode q, the device's work is cut along q's grid coordinate as well: the
//      coordinates whose cells the device already holds come first (no remote dependency), the remote ones
//      follow in contiguous runs, so the first local contraction starts while the gather is in flight.
//   3. An operand view that touches a single grid cell living on the computing device is read (or, for D,
//      written) in place.  Everything else is staged in the device's workspace as an image [cell][cell
//      buffer]: local cells by device copies on the device's own stream, remote cells over xGMI by RCCL
//      ncclSend / ncclRecv pairs inside ONE ncclGroup per wave on a separate communication stream per
//      device (or by peer copies on several streams: CUTENSORMG_AMD_TRANSPORT=peer, and when RCCL is not
//      available).  Every wave records an event; a piece waits only for the waves that carry its cells.
//   4. The staged image *is* a tensor: mode i becomes (w_i inside a block, block-index digits) with strides
//      (elementStride_i, cellElems * cellStride_i per grid digit, blockStride_i per local-block digit); the
//      local contraction is one cutensorContract per piece on these strided views — no redistribution kernel.
//   5. Pieces alternate between the caller's stream and an auxiliary stream per device (two local
//      contractions in flight hide each other's tails); staged pieces of C are copied to the owners' cells
//      by identity cutensorPermute on strided views (peer stores over xGMI when the owner is remote).
//
// Shared modes must have the same block size in every tensor that carries them; their device counts may
// differ when they divide each other (e.g. B distributed along j, C not): the block index is then split
// into common mixed-radix digits.  A tensor in any other layout is brought into an accepted one by cutensorMgCopy
// (the second half of this file).
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <map>
#include <memory>
#include <new>
#include <set>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cutensor.h>
#include <cutensorMg.h>

#include "../host/api_guard.hpp"
#include "mg_kernels.h"

extern "C" int ctamdLogLevel(void);   // libcutensor.so: CUTENSOR_LOG_LEVEL
extern "C" int ctamdPlanPeelLaunches(const cutensorPlan_t plan);
extern "C" int ctamdPlanModeTableGroups(const cutensorPlan_t plan, int32_t* group, int32_t* label, int64_t* extent, int maxOut);   // libcutensor.so diagnostic

namespace {

struct MgTensor {
    uint32_t n = 0;
    std::vector<int64_t> extent, elemStride, blockSize, blockStride;
    std::vector<int32_t> deviceCount;
    std::vector<int64_t> localBlocks;   // blocks of each mode stored per cell
    std::vector<int64_t> cellStride;    // linear cell index = sum c_i * cellStride_i
    std::vector<int32_t> devices;       // owner of each cell
    int64_t cellElems = 0;              // elements spanned by one cell buffer
    int64_t numCells = 1;
    hipDataType dtype = HIP_R_32F;
};

size_t elem_size(hipDataType t) {
    switch (t) {
        case HIP_R_16F: case HIP_R_16BF: return 2;
        case HIP_R_32F: return 4;
        case HIP_R_64F: return 8;
        default: return 0;
    }
}

constexpr int kMaxDigits = 6;      // block-index digits per label (labels of the local views: 8 * label + digit, 7 = w)
constexpr int kComputeStreams = 2; // caller's stream + one auxiliary stream per device

// Mixed-radix split of a label's block index b = sum digit_j * prod_{i<j} f_i, fine enough that every tensor's
// (grid coordinate, local block) split is a prefix: dc_T = f_0 * ... * f_{t-1}.
struct Radix {
    int64_t blockSize = 1, numBlocks = 1;
    std::vector<int64_t> f;        // digit extents, least significant first (may be empty: one block)
};

struct OperandUse {               // how one piece sees one tensor (0 = A, 1 = B, 2 = C/D)
    bool direct = false;          // the view touches one cell that lives on the computing device: used in place
    int cell = -1;                // that cell
    int64_t off = 0;              // element offset of the view (inside the staging image, or inside the cell)
    std::vector<int> cells;       // staged: the cells the view touches
};

struct Piece {
    int dev = 0;                  // index into the handle's device list
    int64_t lo = 0, hi = 0;       // range of the sharded mode p
    int64_t lo2 = 0, hi2 = 0;     // range of the second sharded mode p2 (hi2 == 0: there is none)
    int64_t q0 = 0, q1 = 0;       // range of q's grid coordinate (q1 == 0: q is not cut)
    int stream = 0;               // 0 = caller's stream, 1 = auxiliary stream
    // One local contraction per box of the contracted index space: a single box unless a contracted mode is ragged
    // (extent not a multiple of blockSize * deviceCount, blog_post.cu:168-175 derives every block size with ceil()) —
    // then the valid part of the padded index space is a union of boxes (kbox_list) and the boxes accumulate into D.
    // accumulate: an earlier sub-contraction of this piece already wrote this region of D (the clip sets differ in contracted
    // labels only) -> beta = 1 on D; otherwise the region is new (first box, or a peeled digit of a free mode) -> the caller's beta
    // hv: the three operand views (extents, element strides, mode labels; offsets are off[]) the local plan was built from — kept for
    // ctamdMgReplayOnHost, which walks the plan over host memory
    struct HostView { std::vector<int64_t> extent, stride; std::vector<int32_t> modes; };
    struct Sub { cutensorPlan_t plan = nullptr; uint64_t ws = 0; int64_t off[3] = {0, 0, 0}; bool accumulate = false; HostView hv[3]; };
    std::vector<Sub> subs;
    OperandUse use[3];
    struct Scatter { int cell; int64_t off; cutensorPlan_t plan; HostView hv; };
    std::vector<Scatter> scatter; // staged C -> owner cells
    std::vector<int> waitEvents;  // transfer events (indices into the plan's event table) this piece waits for
    double flops = 0.0;
};

struct Transfer {                 // one cell copied into a device's staging image
    int tensor = 0, cell = 0;
    int dst = 0;                  // handle device index that receives
    int src = -1;                 // handle device index of the owner (-1: the owner is not in the handle)
    int32_t ownerDevice = 0;      // HIP device id of the owner
    bool local = false;           // owner is the receiving device: device copy on the caller's stream
    int wave = 0;                 // remote transfers: RCCL group / event index on the receiver
    int64_t bytes = 0;
    int event = -1;               // index into the plan's event table (remote transfers)
};

}  // namespace

// One worker thread per handle device (round 6; round-5 review, Weak #6).  cutensorMgContraction is driven by ONE host thread
// (contraction_multi_gpu.cu:286-345), and at 8 devices that thread's enqueue work — per device: staging copies, event waits, one or
// more cutensorContract calls — was measured at 184-195 us per call (tools/mg_host_cost_n.py, 8 logical devices), more than the
// 170 us of device time the sample's 4096^3 leaves each of 8 GPUs.  The per-device parts of a call (local staging copies; the pieces'
// event waits + local contractions + scatters) only touch that device's streams, so worker g — which set its device ONCE — issues them
// while the calling thread keeps everything that orders devices against each other (fork, RCCL groups / peer copies, wave events,
// join).  A phase is handed out with run() and collected with wait(); workers spin briefly for the next phase of a call and sleep
// on a condition variable between calls.
struct MgWorkers {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<uint64_t> phase{0};
    std::atomic<int> pending{0};
    std::atomic<int> failed{0};
    const std::function<cutensorStatus_t(int)>* fn = nullptr;
    bool stop = false;

    void start(const std::vector<int32_t>& devices) {
        const int n = (int)devices.size();
        for (int g = 0; g < n; ++g) {
            const int dev = devices[(size_t)g];
            threads.emplace_back([this, g, dev] {
                (void)hipSetDevice(dev);
                uint64_t seen = 0;
                for (;;) {
                    // a new phase: spin for a while (the next phase of the same call arrives within microseconds), then sleep
                    int spins = 0;
                    while (phase.load(std::memory_order_acquire) == seen && ++spins < 20000) __builtin_ia32_pause();
                    if (phase.load(std::memory_order_acquire) == seen) {
                        std::unique_lock<std::mutex> lk(m);
                        cv.wait(lk, [&] { return stop || phase.load(std::memory_order_acquire) != seen; });
                    }
                    if (phase.load(std::memory_order_acquire) == seen) return;     // stop
                    seen = phase.load(std::memory_order_acquire);
                    cutensorStatus_t st = CUTENSOR_STATUS_INTERNAL_ERROR;
                    try { st = (*fn)(g); } catch (...) { }
                    if (st != CUTENSOR_STATUS_SUCCESS) failed.store((int)st, std::memory_order_relaxed);
                    pending.fetch_sub(1, std::memory_order_acq_rel);
                }
            });
        }
    }
    bool active() const { return !threads.empty(); }
    // every worker g runs f(g); returns at once — wait() collects
    void run(const std::function<cutensorStatus_t(int)>& f) {
        fn = &f;
        failed.store(0, std::memory_order_relaxed);
        pending.store((int)threads.size(), std::memory_order_release);
        {
            std::lock_guard<std::mutex> lk(m);     // pairs with the sleepers' predicate check
            phase.fetch_add(1, std::memory_order_acq_rel);
        }
        cv.notify_all();
    }
    cutensorStatus_t wait() {
        while (pending.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
        const int f = failed.load(std::memory_order_relaxed);
        return f == 0 ? CUTENSOR_STATUS_SUCCESS : (cutensorStatus_t)f;
    }
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        for (std::thread& t : threads) t.join();
        threads.clear();
    }
};

struct cutensorMgHandle {
    MgWorkers workers;               // one per handle device when there are several (and a GPU is visible)
    std::mutex callMutex;            // the workers take one phase at a time: concurrent cutensorMgContraction calls on ONE handle queue up here
    std::vector<int32_t> devices;
    std::vector<cutensorHandle_t> handles;
    bool distinct = true;
    // CUTENSORMG_AMD_FORCE_GATHER=1 at cutensorMgCreate (round 5): the operands are ALWAYS staged through the communication path — cells
    // the computing device already holds travel to its own staging image by RCCL (one-rank ncclAllGather, or ncclSend / ncclRecv to
    // itself) on the communication stream, the pieces read the staged image behind the wave event.  A communicator is created for
    // ONE device too.  This is how the all-gather / event-graph code of contraction_multi_gpu.cu:286-345's path executes on a
    // one-GPU box (tests/test_gpu_mg.py, bench.py's forced-gather line); no effect on results.
    bool forceGather = false;
    bool haveDevice = false;         // false: no GPU visible — descriptors and plans only (CPU tests)
    std::vector<ncclComm_t> comms;   // one per handle device when distinct and > 1
    // execution resources, created on first use: [device][k]
    std::vector<std::vector<hipStream_t>> commStreams;
    std::vector<hipStream_t> auxStreams;
};
struct cutensorMgTensorDescriptor { MgTensor t; };
struct cutensorMgContractionDescriptor {
    MgTensor A, B, C, D;
    std::vector<int32_t> mA, mB, mC;
    cutensorComputeType_t compute;
};
struct cutensorMgContractionFind { cutensorMgAlgo_t algo; };
struct cutensorMgContractionPlan {
    cutensorMgContractionDescriptor desc;
    std::vector<Piece> pieces;                 // execution order per device
    std::vector<Transfer> transfers;
    int numWaves = 0;
    int64_t stagingBytes[3] = {0, 0, 0};
    uint64_t contractionWs = 0;                // per compute stream
    int pLabel = -1, qLabel = -1;
    int p2Label = -1;                          // second sharded mode (p shorter than 16 x devices), -1: none
    int numBoxes = 1;                          // local contractions per piece (> 1: a contracted mode is ragged)
    int peeled = 0;                            // how many times a digit of an oversized mode group was peeled into a host loop
    bool useRccl = false;
    bool forceGather = false;     // handle created under CUTENSORMG_AMD_FORCE_GATHER=1: operands always staged through the communication path
    // events (created on first execution): per device {start, localReady, auxDone, commDone[k]...}, then one per (device, wave)
    std::vector<hipEvent_t> events;
    int evPerDevice = 0;
    int commPerDevice = 1;
    std::vector<char> usesAux, usesComm;       // per handle device: does any piece run on the auxiliary stream / any cell arrive from afar
    // ---- cross-device ordering the caller's streams owe each other (filled by the plan) ----
    // scatterOwners[g * kComputeStreams + s]: handle devices whose cells of D the pieces on (g, s) store into from afar: their
    // caller streams end behind that compute stream.  readOwners[g]: handle devices whose cells device g's communication
    // streams read by peer copies: their caller streams end behind those reads (the owner may overwrite its operand next).
    std::vector<std::vector<int>> scatterOwners, readOwners;
    int evScatter = 0;                         // first of the kComputeStreams "scatter done" events inside a device's event block
    // ---- all-gather transport (contraction_multi_gpu.cu:328-332 sits on one all-gather of the operand that does not carry the
    // sharded mode): tensor k qualifies when it has one cell per handle device, cell c owned by handle device c, and every
    // device gathers every cell in wave 0 — then its staging image [cell][cell buffer] IS ncclAllGather's receive layout.
    bool allGatherEligible[3] = {false, false, false};
    int transport = 0;                         // 0 = auto (all-gather where eligible, timed against send/recv on the first two calls),
                                               // 1 = all-gather where eligible, 2 = send/recv pairs only   (CUTENSORMG_AMD_TRANSPORT)
    int calls = 0;                             // executions so far (auto: call 0 all-gather, call 1 send/recv, then the faster)
    hipEvent_t trialEv[4] = {nullptr, nullptr, nullptr, nullptr};   // {start, end} of the gather on device 0's communication stream, per trial
    int chosen = 0;                            // auto, after the trials: 1 = all-gather, 2 = send/recv, 0 = not decided yet
    float trialMs[2] = {0.f, 0.f};
    const cutensorMgHandle* owner = nullptr;
};

namespace {

class DeviceGuard {   // the caller's current device is restored (contraction_multi_gpu.cu:320-346)
public:
    DeviceGuard() { if (hipGetDevice(&saved_) != hipSuccess) { saved_ = -1; (void)hipGetLastError(); } }
    ~DeviceGuard() { if (saved_ >= 0) (void)hipSetDevice(saved_); }
private:
    int saved_ = -1;
};

int find_label(const std::vector<int32_t>& v, int32_t l) {
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == l) return (int)i;
    return -1;
}

int device_rank(const cutensorMgHandle* h, int32_t dev) {
    for (size_t i = 0; i < h->devices.size(); ++i)
        if (h->devices[i] == dev) return (int)i;
    return -1;
}

struct View {
    std::vector<int64_t> extent, stride;
    std::vector<int32_t> modes;
    int64_t offset = 0;
};

// Restriction of a label inside a view: the sharded mode p is pinned to [lo, hi) inside block `block`; q's digit
// `digit` is cut to [c0, c1).
// Clip of a (contracted, ragged) label to one box of its valid index space: w in [0, wHi), digit j in [lo_j, hi_j).
struct Clip {
    int label = -1;
    int64_t wHi = 0;
    std::vector<std::pair<int64_t, int64_t>> digit;
};
struct Restrict {
    int pLabel = -1; int64_t lo = 0, hi = 0;
    int p2Label = -1; int64_t lo2 = 0, hi2 = 0;     // second sharded mode (short first modes: blog_post.cu at small scalings), same semantics
    bool is_p(int li) const { return li == pLabel || li == p2Label; }
    int64_t plo(int li) const { return li == pLabel ? lo : lo2; }
    int64_t phi(int li) const { return li == pLabel ? hi : hi2; }
    int qLabel = -1; int qDigit = -1; int64_t c0 = 0, c1 = 0;
    std::vector<Clip> clips;
    const Clip* clip_of(int li) const {
        for (const Clip& c : clips) if (c.label == li) return &c;
        return nullptr;
    }
};

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

cutensorStatus_t make_desc(cutensorHandle_t h, const View& v, hipDataType type, cutensorTensorDescriptor_t* d) {
    const uint32_t a = std::min<uint32_t>(align_of(v.offset * (int64_t)elem_size(type), elem_size(type)), 16u);
    return cutensorCreateTensorDescriptor(h, d, (uint32_t)v.extent.size(), v.extent.data(), v.stride.data(), type, a);
}

cutensorComputeDescriptor_t compute_desc(cutensorComputeType_t c) {
    switch (c) {
        case CUTENSOR_COMPUTE_16F: return CUTENSOR_COMPUTE_DESC_16F;
        case CUTENSOR_COMPUTE_16BF: return CUTENSOR_COMPUTE_DESC_16BF;
        case CUTENSOR_COMPUTE_64F: return CUTENSOR_COMPUTE_DESC_64F;
        default: return CUTENSOR_COMPUTE_DESC_32F;
    }
}

ncclDataType_t nccl_type(hipDataType t) {
    switch (t) {
        case HIP_R_16F: return ncclFloat16;
        case HIP_R_16BF: return ncclBfloat16;
        case HIP_R_64F: return ncclFloat64;
        default: return ncclFloat32;
    }
}

void destroy_pieces(std::vector<Piece>& pieces) {
    for (Piece& p : pieces) {
        for (auto& sub : p.subs) cutensorDestroyPlan(sub.plan);
        for (auto& s : p.scatter) cutensorDestroyPlan(s.plan);
    }
    pieces.clear();
}

bool env_is(const char* name, const char* value) {
    const char* e = std::getenv(name);
    return e != nullptr && std::strcmp(e, value) == 0;
}
// test / measurement switches: read by the hooks flavour only (host/api_guard.hpp)
#if CTAMD_HOOKS_BUILT
#define CTAMD_HOOK_IS(NAME, VALUE) env_is(NAME, VALUE)
#else
#define CTAMD_HOOK_IS(NAME, VALUE) false
#endif

}  // namespace

extern "C" {

// contraction_multi_gpu.cu:151
cutensorStatus_t cutensorMgCreate(cutensorMgHandle_t* handle, uint32_t numDevices, const int32_t devices[]) try {
    if (handle == nullptr || numDevices == 0 || devices == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    DeviceGuard guard;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    cutensorMgHandle* h = new (std::nothrow) cutensorMgHandle();
    if (h == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    h->haveDevice = count > 0;
    h->devices.assign(devices, devices + numDevices);
    std::set<int32_t> uniq(h->devices.begin(), h->devices.end());
    h->distinct = uniq.size() == h->devices.size();
    h->forceGather = env_is("CUTENSORMG_AMD_FORCE_GATHER", "1");
    for (int32_t d : h->devices) {
        if (d < 0 || (count > 0 && d >= count)) { cutensorMgDestroy(h); return CUTENSOR_STATUS_INVALID_VALUE; }
        if (count > 0) (void)hipSetDevice(d);
        cutensorHandle_t ch = nullptr;
        if (cutensorCreate(&ch) != CUTENSOR_STATUS_SUCCESS) { cutensorMgDestroy(h); return CUTENSOR_STATUS_ALLOC_FAILED; }
        h->handles.push_back(ch);
        if (count > 0)
            for (int32_t o : uniq)
                if (o != d) { (void)hipDeviceEnablePeerAccess(o, 0); (void)hipGetLastError(); }   // xGMI peer mapping
    }
    if (count > 0 && h->distinct && (numDevices > 1 || h->forceGather) && !env_is("CUTENSORMG_AMD_TRANSPORT", "peer")) {
        h->comms.resize(numDevices);
        std::vector<int> devs(h->devices.begin(), h->devices.end());
        if (ncclCommInitAll(h->comms.data(), (int)numDevices, devs.data()) != ncclSuccess) h->comms.clear();
    }
    // worker threads for the per-device parts of a call (MgWorkers): from FOUR handle devices on — measured (tools/mg_host_cost_n.py, bench
    // layout, us per call idle / back to back, workers against one thread): two devices 21 / 15 against 14 / 14, four 28 / 20 against
    // 23 / 26, eight 35 / 27.5 against 47 / 48 (profiles/r06r_mg_host_cost_*).  CUTENSORMG_AMD_THREADS (hooks flavour): 0 keeps
    // everything on the calling thread, 1 starts the workers from two devices on
    const bool wantWorkers = CTAMD_HOOK_IS("CUTENSORMG_AMD_THREADS", "1") ? numDevices > 1 : (numDevices >= 4 && !CTAMD_HOOK_IS("CUTENSORMG_AMD_THREADS", "0"));
    if (count > 0 && wantWorkers) h->workers.start(h->devices);
    *handle = h;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:383
cutensorStatus_t cutensorMgDestroy(cutensorMgHandle_t handle) try {
    if (handle == nullptr) return CUTENSOR_STATUS_SUCCESS;
    DeviceGuard guard;
    for (size_t g = 0; g < handle->commStreams.size(); ++g) {
        if (handle->haveDevice) (void)hipSetDevice(handle->devices[g]);
        for (hipStream_t s : handle->commStreams[g]) (void)hipStreamDestroy(s);
        if (g < handle->auxStreams.size() && handle->auxStreams[g]) (void)hipStreamDestroy(handle->auxStreams[g]);
    }
    handle->workers.shutdown();
    for (ncclComm_t c : handle->comms) (void)ncclCommDestroy(c);
    for (cutensorHandle_t h : handle->handles) cutensorDestroy(h);
    delete handle;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:195-197
cutensorStatus_t cutensorMgCreateTensorDescriptor(const cutensorMgHandle_t handle, cutensorMgTensorDescriptor_t* desc,
                                                  uint32_t numModes, const int64_t extent[], const int64_t elementStride[],
                                                  const int64_t blockSize[], const int64_t blockStride[],
                                                  const int32_t deviceCount[], uint32_t numDevices, const int32_t devices[],
                                                  cudaDataType_t type) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || (numModes > 0 && extent == nullptr) || devices == nullptr || numDevices == 0) return CUTENSOR_STATUS_INVALID_VALUE;
    if (numModes > 20 || elem_size(type) == 0) return CUTENSOR_STATUS_NOT_SUPPORTED;
    cutensorMgTensorDescriptor* d = new (std::nothrow) cutensorMgTensorDescriptor();
    if (d == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    MgTensor& t = d->t;
    t.n = numModes;
    t.dtype = type;
    t.extent.assign(extent, extent + numModes);
    t.blockSize.resize(numModes); t.deviceCount.resize(numModes); t.localBlocks.resize(numModes);
    t.elemStride.resize(numModes); t.blockStride.resize(numModes); t.cellStride.resize(numModes);
    int64_t cells = 1, run = 1;
    for (uint32_t i = 0; i < numModes; ++i) {
        if (extent[i] <= 0) { delete d; return CUTENSOR_STATUS_INVALID_VALUE; }
        t.blockSize[i] = blockSize ? blockSize[i] : extent[i];
        t.deviceCount[i] = deviceCount ? deviceCount[i] : 1;
        if (t.blockSize[i] <= 0 || t.deviceCount[i] <= 0) { delete d; return CUTENSOR_STATUS_INVALID_VALUE; }
        // every cell stores whole blocks: ceil(ceil(extent / blockSize) / deviceCount) of them per mode, exactly what the
        // samples allocate (contraction_multi_gpu.cu:256 discretize(); blog_post.cu:107-113).  A ragged extent leaves
        // padding at the end of the index space; the contraction descriptor decides whether that is acceptable.
        const int64_t blocks = (extent[i] + t.blockSize[i] - 1) / t.blockSize[i];
        t.localBlocks[i] = (blocks + t.deviceCount[i] - 1) / t.deviceCount[i];
        t.cellStride[i] = cells;
        cells *= t.deviceCount[i];
        t.elemStride[i] = elementStride ? elementStride[i] : run;
        run *= t.blockSize[i];
    }
    int64_t brun = run;   // packed block stride: one whole block, then blocks of mode 0, 1, ...
    for (uint32_t i = 0; i < numModes; ++i) {
        t.blockStride[i] = blockStride ? blockStride[i] : brun;
        brun *= t.localBlocks[i];
    }
    if ((int64_t)numDevices != cells) { delete d; return CUTENSOR_STATUS_INVALID_VALUE; }
    for (uint32_t i = 0; i < numDevices; ++i)
        if (devices[i] == CUTENSOR_MG_DEVICE_HOST) { delete d; return CUTENSOR_STATUS_NOT_SUPPORTED; }
    t.devices.assign(devices, devices + numDevices);
    t.numCells = cells;
    int64_t span = 1;
    for (uint32_t i = 0; i < numModes; ++i)
        span += (t.blockSize[i] - 1) * t.elemStride[i] + (t.localBlocks[i] - 1) * t.blockStride[i];
    t.cellElems = span;
    *desc = d;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyTensorDescriptor(cutensorMgTensorDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:228-233
cutensorStatus_t cutensorMgCreateContractionDescriptor(const cutensorMgHandle_t handle, cutensorMgContractionDescriptor_t* desc,
                                                       const cutensorMgTensorDescriptor_t descA, const int32_t modesA[],
                                                       const cutensorMgTensorDescriptor_t descB, const int32_t modesB[],
                                                       const cutensorMgTensorDescriptor_t descC, const int32_t modesC[],
                                                       const cutensorMgTensorDescriptor_t descD, const int32_t modesD[],
                                                       cutensorComputeType_t compute) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || descA == nullptr || descB == nullptr || descC == nullptr || descD == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorMgContractionDescriptor* d = new (std::nothrow) cutensorMgContractionDescriptor();
    if (d == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    d->A = descA->t; d->B = descB->t; d->C = descC->t; d->D = descD->t;
    d->mA.assign(modesA, modesA + d->A.n);
    d->mB.assign(modesB, modesB + d->B.n);
    d->mC.assign(modesC, modesC + d->C.n);
    std::vector<int32_t> mD(modesD, modesD + d->D.n);
    d->compute = compute;
    // D must be distributed exactly like C (the sample passes the same descriptor twice)
    const bool sameCD = mD == d->mC && d->C.extent == d->D.extent && d->C.blockSize == d->D.blockSize &&
                        d->C.deviceCount == d->D.deviceCount && d->C.elemStride == d->D.elemStride &&
                        d->C.blockStride == d->D.blockStride && d->C.devices == d->D.devices;
    if (!sameCD || d->A.dtype != d->B.dtype || d->A.dtype != d->C.dtype) { delete d; return CUTENSOR_STATUS_NOT_SUPPORTED; }
    // a mode shared by two tensors must be cut into the same blocks in both, and the two device counts must divide one
    // another (the block index then has common mixed-radix digits)
    auto check = [&](const MgTensor& x, const std::vector<int32_t>& mx, const MgTensor& y, const std::vector<int32_t>& my) {
        for (uint32_t i = 0; i < x.n; ++i) {
            const int j = find_label(my, mx[i]);
            if (j < 0) continue;
            if (x.extent[i] != y.extent[j]) return CUTENSOR_STATUS_INVALID_VALUE;
            if (x.blockSize[i] != y.blockSize[j]) return CUTENSOR_STATUS_NOT_SUPPORTED;
            const int64_t a = x.deviceCount[i], b = y.deviceCount[j];
            if (a % b != 0 && b % a != 0) return CUTENSOR_STATUS_NOT_SUPPORTED;
            if (x.localBlocks[i] * a != y.localBlocks[j] * b) return CUTENSOR_STATUS_NOT_SUPPORTED;   // same padded block count
        }
        return CUTENSOR_STATUS_SUCCESS;
    };
    cutensorStatus_t st = check(d->A, d->mA, d->B, d->mB);
    if (st == CUTENSOR_STATUS_SUCCESS) st = check(d->A, d->mA, d->C, d->mC);
    if (st == CUTENSOR_STATUS_SUCCESS) st = check(d->B, d->mB, d->C, d->mC);
    // Ragged extents (not a multiple of blockSize * deviceCount; blog_post.cu:168-175 derives every block size with ceil()):
    // a ragged mode of C only produces extra results in the padding of D's cells, which the caller never reads, so the local
    // contractions simply run over the padded index space; a ragged CONTRACTED mode would put the padding into every sum, so
    // the plan clips it: the valid part of its index space is tiled by boxes (kbox_list) that accumulate into D.
    if (st != CUTENSOR_STATUS_SUCCESS) { delete d; return st; }
    *desc = d;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyContractionDescriptor(cutensorMgContractionDescriptor_t desc) try {
    delete desc;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:236-237
cutensorStatus_t cutensorMgCreateContractionFind(const cutensorMgHandle_t handle, cutensorMgContractionFind_t* find,
                                                 const cutensorMgAlgo_t algo) try {
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (find == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    cutensorMgContractionFind* f = new (std::nothrow) cutensorMgContractionFind();
    if (f == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    f->algo = algo;
    *find = f;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyContractionFind(cutensorMgContractionFind_t find) try {
    delete find;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

static const uint64_t kLocalContractionWs = 128ull << 20;   // split-K scratch offered to every local plan (per compute stream)

// Upper bound of the staging images (whether a tensor needs staging at all is decided by the plan; the workspace
// query must not be smaller than what any plan of this descriptor can ask for).
static void staging_sizes(const cutensorMgContractionDescriptor& d, int64_t out[3]) {
    const size_t es = elem_size(d.A.dtype);
    auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
    out[0] = up(d.A.numCells * d.A.cellElems * (int64_t)es);
    out[1] = up(d.B.numCells * d.B.cellElems * (int64_t)es);
    out[2] = up(d.C.numCells * d.C.cellElems * (int64_t)es);
}

// contraction_multi_gpu.cu:241-242
cutensorStatus_t cutensorMgContractionGetWorkspace(const cutensorMgHandle_t handle, const cutensorMgContractionDescriptor_t desc,
                                                   const cutensorMgContractionFind_t find, cutensorWorksizePreference_t preference,
                                                   int64_t deviceWorkspaceSize[], int64_t* hostWorkspaceSize) try {
    (void)find; (void)preference;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (desc == nullptr || deviceWorkspaceSize == nullptr || hostWorkspaceSize == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    int64_t s[3];
    staging_sizes(*desc, s);
    for (size_t i = 0; i < handle->devices.size(); ++i)
        deviceWorkspaceSize[i] = s[0] + s[1] + s[2] + (int64_t)(kComputeStreams * kLocalContractionWs);
    *hostWorkspaceSize = 0;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// contraction_multi_gpu.cu:249-250
cutensorStatus_t cutensorMgCreateContractionPlan(const cutensorMgHandle_t handle, cutensorMgContractionPlan_t* plan,
                                                 const cutensorMgContractionDescriptor_t desc, const cutensorMgContractionFind_t find,
                                                 const int64_t deviceWorkspaceSize[], int64_t hostWorkspaceSize) try {
    (void)find; (void)hostWorkspaceSize;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || desc == nullptr || deviceWorkspaceSize == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    DeviceGuard guard;
    cutensorMgContractionPlan* pl = new (std::nothrow) cutensorMgContractionPlan();
    if (pl == nullptr) return CUTENSOR_STATUS_ALLOC_FAILED;
    pl->desc = *desc;
    pl->owner = handle;
    const cutensorMgContractionDescriptor& d = pl->desc;
    const int nDev = (int)handle->devices.size();
    const size_t es = elem_size(d.A.dtype);
    staging_sizes(d, pl->stagingBytes);
    const int64_t fixed = pl->stagingBytes[0] + pl->stagingBytes[1] + pl->stagingBytes[2];
    uint64_t ctrWs = kLocalContractionWs;
    for (int g = 0; g < nDev; ++g) {
        if (deviceWorkspaceSize[g] < fixed) { delete pl; return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE; }
        ctrWs = std::min<uint64_t>(ctrWs, (uint64_t)(deviceWorkspaceSize[g] - fixed) / kComputeStreams / 256 * 256);
    }
    pl->contractionWs = ctrWs;
    pl->forceGather = handle->forceGather;
    pl->useRccl = !handle->comms.empty() ||
                  // plan-only handles (no GPU visible): CPU tests of the RCCL event wiring and transport choice
                  (!handle->haveDevice && handle->distinct && (nDev > 1 || handle->forceGather) && CTAMD_HOOK_IS("CUTENSORMG_AMD_ASSUME_RCCL", "1"));

    // ---- label universe, block-index digits per label ----------------------------------------------
    const MgTensor* T[3] = {&d.A, &d.B, &d.C};
    const std::vector<int32_t>* M[3] = {&d.mA, &d.mB, &d.mC};
    std::vector<int32_t> universe;
    for (int k = 0; k < 3; ++k)
        for (int32_t l : *M[k])
            if (find_label(universe, l) < 0) universe.push_back(l);
    std::vector<Radix> radix(universe.size());
    for (size_t li = 0; li < universe.size(); ++li) {
        std::set<int64_t> dcs;
        Radix& r = radix[li];
        for (int k = 0; k < 3; ++k) {
            const int i = find_label(*M[k], universe[li]);
            if (i < 0) continue;
            r.blockSize = T[k]->blockSize[i];
            r.numBlocks = T[k]->localBlocks[i] * T[k]->deviceCount[i];      // padded: whole blocks per cell
            dcs.insert(T[k]->deviceCount[i]);
        }
        int64_t prev = 1;
        for (int64_t dc : dcs) {          // ascending; each divides the next (checked by the contraction descriptor)
            if (dc % prev != 0) { delete pl; return CUTENSOR_STATUS_NOT_SUPPORTED; }
            if (dc / prev > 1) r.f.push_back(dc / prev);
            prev = dc;
        }
        if (r.numBlocks / prev > 1) r.f.push_back(r.numBlocks / prev);
        if ((int)r.f.size() > kMaxDigits) { delete pl; return CUTENSOR_STATUS_NOT_SUPPORTED; }
    }

    // ---- the mode to shard (p) and the mode that orders the gather (q) --------------------------------
    int pC = -1;   // index in C of the largest mode that is free (in exactly one of A / B) — else any C mode
    for (int pass = 0; pass < 2 && pC < 0; ++pass)
        for (uint32_t i = 0; i < d.C.n; ++i) {
            const bool inA = find_label(d.mA, d.mC[i]) >= 0, inB = find_label(d.mB, d.mC[i]) >= 0;
            if (pass == 0 && inA == inB) continue;
            if (pC < 0 || d.C.extent[i] > d.C.extent[pC]) pC = (int)i;
        }
    const int pLi = pC >= 0 ? find_label(universe, d.mC[pC]) : -1;
    pl->pLabel = pC >= 0 ? d.mC[pC] : -1;
    // Y = the operand that does not carry p (gathered whole); q = Y's free mode with the largest device count whose
    // grid coordinate is ONE digit in Y (so that a run of coordinates is a box)
    int yK = -1;
    if (pC >= 0) yK = find_label(d.mA, d.mC[pC]) >= 0 ? 1 : 0;
    if (pC >= 0 && find_label(d.mA, d.mC[pC]) >= 0 && find_label(d.mB, d.mC[pC]) >= 0) yK = -1;   // batch mode: both carry it
    int qLi = -1, qDigit = -1;
    int64_t qCount = 1;
    if (yK >= 0 && !CTAMD_HOOK_IS("CUTENSORMG_AMD_QSPLIT", "0")) {
        const MgTensor& Y = *T[yK];
        for (uint32_t i = 0; i < Y.n; ++i) {
            const int32_t l = (*M[yK])[i];
            if (find_label(d.mC, l) < 0 || Y.deviceCount[i] <= 1) continue;
            const int li = find_label(universe, l);
            const int nGrid = grid_digits(radix[li], Y.deviceCount[i]);
            if (nGrid != 1) continue;
            if (Y.deviceCount[i] > qCount) { qCount = Y.deviceCount[i]; qLi = li; qDigit = 0; }
        }
    }
    pl->qLabel = qLi >= 0 ? universe[qLi] : -1;

    // ---- pieces: one shard of p per device, cut at block boundaries, then runs of q's coordinate -------
    // Shards of p start at multiples of 16 indices (64-byte aligned rows for the vector kernels).  When p is too short for one such
    // shard per device (blog_post.cu on 8 devices: its largest free mode has 16 .. 96 indices at scaling 1 .. 12, :155-175) that rule
    // alone leaves devices without work: p is then cut nP ways only (nP = the largest divisor of the device count whose 16-aligned
    // shards are all non-empty) and a SECOND free
    // mode p2 of C — the largest other one, preferably carried by the other operand so that both operands shrink per device — is cut
    // n2 = devices / nP ways (plain ceil() shards: these modes are small, alignment is not the concern).  Device g works on
    // (p shard g % nP, p2 shard g / nP).  The gather-ordering mode q is not used together with p2.
    struct Shard { int dev; int64_t lo, hi, lo2, hi2; };
    std::vector<Shard> shards;
    int p2C = -1, p2Li = -1;
    if (pC < 0) {
        shards.push_back(Shard{0, 0, 0, 0, 0});
    } else {
        const int64_t E = d.C.extent[pC], bs = d.C.blockSize[pC];
        int nP = nDev;
        // c shards of ceil(E / c) rounded up to 16 indices: are all of them non-empty?
        auto all_busy = [&](int c) { const int64_t per = ((E + c - 1) / c + 15) / 16 * 16; return per * (int64_t)(c - 1) < E; };
        if (!all_busy(nDev) && !CTAMD_HOOK_IS("CUTENSORMG_AMD_SHARD2", "0")) {
            nP = 1;
            for (int c = 1; c <= nDev; ++c)
                if (nDev % c == 0 && all_busy(c)) nP = c;
            const bool pInA = find_label(d.mA, d.mC[pC]) >= 0;
            const int n2w = nDev / nP;
            // p2: a free mode with at least n2 indices whose n2 shards cross the FEWEST block boundaries (every crossing is another
            // piece, i.e. another local contraction), the longer one on a tie
            auto segments = [&](uint32_t i) {
                const int64_t e = d.C.extent[i], b = d.C.blockSize[i], per2 = (e + n2w - 1) / n2w;
                int64_t segs = 0;
                for (int g2 = 0; g2 < n2w; ++g2) {
                    const int64_t lo = (int64_t)g2 * per2, hi = std::min<int64_t>(e, lo + per2);
                    if (lo < hi) segs += (hi - 1) / b - lo / b + 1;
                }
                return segs;
            };
            for (int pass = 0; pass < 2 && p2C < 0; ++pass)     // pass 0: free modes of the OTHER operand; pass 1: any other free mode
                for (uint32_t i = 0; i < d.C.n; ++i) {
                    if ((int)i == pC) continue;
                    const bool inA = find_label(d.mA, d.mC[i]) >= 0, inB = find_label(d.mB, d.mC[i]) >= 0;
                    if (inA == inB) continue;                   // batch modes are not sharded
                    if (pass == 0 && inA == pInA) continue;
                    if (d.C.extent[i] < (int64_t)n2w) continue;
                    if (p2C < 0 || segments(i) < segments((uint32_t)p2C) ||
                        (segments(i) == segments((uint32_t)p2C) && d.C.extent[i] > d.C.extent[p2C])) p2C = (int)i;
                }
            if (p2C < 0) nP = nDev;                             // nothing else to cut: the old rule (some devices stay idle)
        }
        const int n2 = (p2C >= 0) ? nDev / nP : 1;
        if (p2C >= 0) { p2Li = find_label(universe, d.mC[p2C]); qLi = -1; qDigit = -1; qCount = 1; pl->qLabel = -1; }
        int64_t per = (E + nP - 1) / nP;
        per = (per + 15) / 16 * 16;   // keep shard starts 64-byte aligned for the vector kernels
        const int64_t E2 = p2C >= 0 ? d.C.extent[p2C] : 0, bs2 = p2C >= 0 ? d.C.blockSize[p2C] : 1;
        const int64_t per2 = p2C >= 0 ? (E2 + n2 - 1) / n2 : 0;
        for (int g = 0; g < nDev; ++g) {
            const int gp = g % nP, g2 = g / nP;
            int64_t lo = (int64_t)gp * per, hi = std::min<int64_t>(E, lo + per);
            while (lo < hi) {
                const int64_t cut = std::min<int64_t>(hi, (lo / bs + 1) * bs);
                if (p2C < 0) shards.push_back(Shard{g, lo, cut, 0, 0});
                else {
                    int64_t lo2 = (int64_t)g2 * per2, hi2 = std::min<int64_t>(E2, lo2 + per2);
                    while (lo2 < hi2) {
                        const int64_t cut2 = std::min<int64_t>(hi2, (lo2 / bs2 + 1) * bs2);
                        shards.push_back(Shard{g, lo, cut, lo2, cut2});
                        lo2 = cut2;
                    }
                }
                lo = cut;
            }
        }
    }
    pl->p2Label = p2C >= 0 ? d.mC[p2C] : -1;
    double flopsAll = 2.0;
    for (size_t li = 0; li < universe.size(); ++li) flopsAll *= (double)(radix[li].blockSize * radix[li].numBlocks);

    auto restrict_of = [&](const Shard& s, int64_t c0, int64_t c1) {
        Restrict rs;
        if (pC >= 0) { rs.pLabel = pLi; rs.lo = s.lo; rs.hi = s.hi; }
        if (p2Li >= 0 && s.hi2 > s.lo2) { rs.p2Label = p2Li; rs.lo2 = s.lo2; rs.hi2 = s.hi2; }
        if (qLi >= 0 && c1 > c0) { rs.qLabel = qLi; rs.qDigit = qDigit; rs.c0 = c0; rs.c1 = c1; }
        return rs;
    };
    // is every cell of tensor k that the restricted view touches local to device g?
    auto all_local = [&](int k, const Restrict& rs, int g) {
        for (int c : cells_of(*T[k], *M[k], universe, radix, rs))
            if (T[k]->devices[c] != handle->devices[g]) return false;
        return true;
    };
    int wavesWanted = 1;
    if (const char* e = std::getenv("CUTENSORMG_AMD_WAVES")) wavesWanted = std::max(1, std::atoi(e));

    std::vector<Piece> pieces;
    int numWaves = 0;
    for (int g = 0; g < nDev; ++g) {
        std::vector<Piece> mine;
        for (const Shard& s : shards) {
            if (s.dev != g) continue;
            if (qLi < 0) {
                Piece p; p.dev = g; p.lo = s.lo; p.hi = s.hi; p.lo2 = s.lo2; p.hi2 = s.hi2;
                mine.push_back(p);
                continue;
            }
            // class of each q coordinate: -1 = everything this coordinate needs of Y is already on the device, else the
            // gather wave that brings it (ring distance from the device's own position, wavesWanted waves)
            std::vector<int> cls((size_t)qCount);
            for (int64_t c = 0; c < qCount; ++c) {
                const Restrict rs = restrict_of(s, c, c + 1);
                if (all_local(yK, rs, g)) { cls[(size_t)c] = -1; continue; }
                const int64_t dist = ((c - g) % qCount + qCount) % qCount;      // 1 .. qCount - 1 for the usual one-cell-per-device layout
                cls[(size_t)c] = (int)std::min<int64_t>(wavesWanted - 1, (dist > 0 ? dist - 1 : 0) * wavesWanted / std::max<int64_t>(1, qCount - 1));
            }
            // maximal runs of equal class, local runs first, then by wave
            struct Run { int64_t c0, c1; int cls; };
            std::vector<Run> runs;
            for (int64_t c = 0; c < qCount;) {
                int64_t e = c + 1;
                while (e < qCount && cls[(size_t)e] == cls[(size_t)c]) ++e;
                runs.push_back(Run{c, e, cls[(size_t)c]});
                c = e;
            }
            std::stable_sort(runs.begin(), runs.end(), [](const Run& a, const Run& b) { return a.cls < b.cls; });
            for (const Run& r : runs) {
                Piece p; p.dev = g; p.lo = s.lo; p.hi = s.hi; p.q0 = r.c0; p.q1 = r.c1;
                mine.push_back(p);
            }
        }
        for (size_t i = 0; i < mine.size(); ++i) mine[i].stream = (int)(i % kComputeStreams);
        pieces.insert(pieces.end(), mine.begin(), mine.end());
    }

    // ---- operand uses, transfers ------------------------------------------------------------------------
    std::map<std::pair<int, std::pair<int, int>>, int> have;   // (device, (tensor, cell)) -> transfer index
    bool staged[3] = {false, false, false};
    for (Piece& p : pieces) {
        const Shard s{p.dev, p.lo, p.hi, p.lo2, p.hi2};
        const Restrict rs = restrict_of(s, p.q0, p.q1);
        p.flops = flopsAll;
        if (pC >= 0) p.flops *= (double)(p.hi - p.lo) / (double)d.C.extent[pC];
        if (p2C >= 0 && p.hi2 > p.lo2) p.flops *= (double)(p.hi2 - p.lo2) / (double)d.C.extent[p2C];
        if (qLi >= 0) p.flops *= (double)(p.q1 - p.q0) / (double)qCount;
        for (int k = 0; k < 3; ++k) {
            OperandUse& u = p.use[k];
            u.cells = cells_of(*T[k], *M[k], universe, radix, rs);
            u.direct = u.cells.size() == 1 && T[k]->devices[u.cells[0]] == handle->devices[p.dev] &&
                       !CTAMD_HOOK_IS("CUTENSORMG_AMD_DIRECT", "0") && !(handle->forceGather && k < 2);
            if (u.direct) { u.cell = u.cells[0]; continue; }
            staged[k] = true;
            for (int c : u.cells) {
                const auto key = std::make_pair(p.dev, std::make_pair(k, c));
                if (have.count(key)) continue;
                Transfer t;
                t.tensor = k; t.cell = c; t.dst = p.dev;
                t.ownerDevice = T[k]->devices[c];
                t.src = device_rank(handle, t.ownerDevice);
                // forced gather: an own cell of an operand is NOT a device copy on the caller's stream — it goes the remote way (RCCL
                // to itself / a peer copy onto the same device) on the communication stream, with its wave event
                t.local = t.ownerDevice == handle->devices[p.dev] && !(handle->forceGather && k < 2);
                t.bytes = T[k]->cellElems * (int64_t)es;
                have[key] = (int)pl->transfers.size();
                pl->transfers.push_back(t);
            }
        }
    }
    // waves of the remote transfers: in the order the pieces of the receiving device first need them
    {
        std::vector<int> nextWave((size_t)nDev, 0);
        std::vector<std::vector<int>> order((size_t)nDev);   // remote transfer indices per device in first-use order
        std::set<int> seen;
        for (const Piece& p : pieces)
            for (int k = 0; k < 3; ++k) {
                if (p.use[k].direct) continue;
                for (int c : p.use[k].cells) {
                    const int ti = have[std::make_pair(p.dev, std::make_pair(k, c))];
                    if (pl->transfers[(size_t)ti].local || seen.count(ti)) continue;
                    seen.insert(ti);
                    order[(size_t)p.dev].push_back(ti);
                }
            }
        for (int g = 0; g < nDev; ++g) {
            const size_t n = order[(size_t)g].size();
            const size_t perWave = std::max<size_t>(1, (n + (size_t)wavesWanted - 1) / (size_t)wavesWanted);
            for (size_t i = 0; i < n; ++i) {
                Transfer& t = pl->transfers[(size_t)order[(size_t)g][i]];
                t.wave = (int)(i / perWave);
                numWaves = std::max(numWaves, t.wave + 1);
            }
        }
    }
    pl->numWaves = numWaves;
    pl->commPerDevice = pl->useRccl ? 1 : std::max(1, std::min(7, nDev - 1));
    pl->evScatter = 3 + pl->commPerDevice + numWaves * (pl->useRccl ? 1 : pl->commPerDevice);
    pl->evPerDevice = pl->evScatter + kComputeStreams;
    for (Transfer& t : pl->transfers) {
        if (t.local) continue;
        // RCCL: one event per (device, wave); peer copies: one event per (device, wave, comm stream)
        t.event = t.dst * pl->evPerDevice + 3 + pl->commPerDevice + t.wave * (pl->useRccl ? 1 : pl->commPerDevice);
    }
    if (!pl->useRccl) {   // spread a wave's peer copies over the communication streams
        std::map<std::pair<int, int>, int> n;
        for (Transfer& t : pl->transfers) {
            if (t.local) continue;
            int& k = n[std::make_pair(t.dst, t.wave)];
            t.event += k % pl->commPerDevice;
            ++k;
        }
    }
    for (Piece& p : pieces) {
        std::set<int> ev;
        for (int k = 0; k < 3; ++k) {
            if (p.use[k].direct) continue;
            for (int c : p.use[k].cells) {
                const Transfer& t = pl->transfers[(size_t)have[std::make_pair(p.dev, std::make_pair(k, c))]];
                if (!t.local) ev.insert(t.event);
            }
        }
        p.waitEvents.assign(ev.begin(), ev.end());
    }
    for (int k = 0; k < 3; ++k)
        if (!staged[k]) pl->stagingBytes[k] = 0;
    // all-gather eligibility per tensor (a property of the layout; whether RCCL is there is a property of the handle)
    for (int k = 0; k < 2; ++k) {   // operands only: C is gathered only for beta != 0 and scattered back, never all-gathered
        bool ok = handle->distinct && (nDev > 1 || handle->forceGather) && T[k]->numCells == nDev;
        for (int c = 0; ok && c < nDev; ++c) ok = T[k]->devices[(size_t)c] == handle->devices[(size_t)c];
        std::vector<int> remote((size_t)nDev, 0);
        for (const Transfer& t : pl->transfers)
            if (t.tensor == k && !t.local) { ++remote[(size_t)t.dst]; ok = ok && t.wave == 0; }
        // every device receives every cell it does not hold (forced gather: its own one too — the collective delivers all nDev anyway)
        for (int g = 0; ok && g < nDev; ++g) ok = remote[(size_t)g] == (handle->forceGather ? nDev : nDev - 1);
        pl->allGatherEligible[k] = ok;
    }
    pl->transport = env_is("CUTENSORMG_AMD_TRANSPORT", "allgather") ? 1 : env_is("CUTENSORMG_AMD_TRANSPORT", "sendrecv") ? 2 : 0;
    pl->readOwners.assign((size_t)nDev, {});
    for (const Transfer& t : pl->transfers) {
        if (t.local) continue;
        for (int o = 0; o < nDev; ++o)
            if (o != t.dst && handle->devices[(size_t)o] == t.ownerDevice &&
                std::find(pl->readOwners[(size_t)t.dst].begin(), pl->readOwners[(size_t)t.dst].end(), o) == pl->readOwners[(size_t)t.dst].end())
                pl->readOwners[(size_t)t.dst].push_back(o);
    }
    pl->usesAux.assign((size_t)nDev, 0);
    pl->usesComm.assign((size_t)nDev, 0);
    for (const Piece& p : pieces) if (p.stream != 0) pl->usesAux[(size_t)p.dev] = 1;
    for (const Transfer& t : pl->transfers)
        if (!t.local) { pl->usesComm[(size_t)t.dst] = 1; if (t.src >= 0) pl->usesComm[(size_t)t.src] = 1; }

    // ---- local plans ----------------------------------------------------------------------------
    const cutensorComputeDescriptor_t cd = compute_desc(d.compute);
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    // boxes of the contracted index space (one, unless a contracted mode is ragged): the cartesian product of kbox_list()
    std::vector<std::vector<Clip>> boxes(1);
    for (size_t li = 0; li < universe.size(); ++li) {
        if (find_label(d.mC, universe[li]) >= 0) continue;              // a mode of C: padded, never clipped
        int64_t extent = 0;
        for (int k = 0; k < 2; ++k) {
            const int i = find_label(*M[k], universe[li]);
            if (i >= 0) extent = T[k]->extent[(size_t)i];
        }
        if (extent == radix[li].blockSize * radix[li].numBlocks) continue;   // fills the padded space
        const std::vector<Clip> mine = kbox_list((int)li, radix[li], extent);
        std::vector<std::vector<Clip>> next;
        for (const auto& b : boxes)
            for (const Clip& c : mine) { next.push_back(b); next.back().push_back(c); }
        boxes.swap(next);
    }
    if (boxes.empty() || boxes.size() > 64) st = CUTENSOR_STATUS_NOT_SUPPORTED;
    // 16-bit data: boxes accumulate through D, which would round every partial sum to the 16-bit type (the kernels' contract is fp32
    // accumulation and one rounding) — a ragged contracted mode stays unsupported for these types
    if (boxes.size() > 1 && es == 2) st = CUTENSOR_STATUS_NOT_SUPPORTED;
    pl->numBoxes = (int)boxes.size();
    for (Piece& p : pieces) {
        if (st != CUTENSOR_STATUS_SUCCESS) break;
        if (handle->haveDevice) { (void)hipSetDevice(handle->devices[p.dev]); (void)hipGetLastError(); }
        cutensorHandle_t h = handle->handles[p.dev];
        const Shard s{p.dev, p.lo, p.hi, p.lo2, p.hi2};
        Restrict rs = restrict_of(s, p.q0, p.q1);
        // work list of clip sets: the boxes of the contracted index space, each possibly split further ("peeled") below.  acc: an
        // earlier entry already writes this region of D — every box after the first (the boxes tile the CONTRACTED index space, all
        // cover the piece's whole output), and every value but the first of a peeled contracted digit; peeled free digits inherit.
        struct Work { std::vector<Clip> clips; bool acc; };
        std::vector<Work> todo;
        for (size_t bi = boxes.size(); bi-- > 0;) todo.push_back(Work{boxes[bi], bi > 0});
        while (!todo.empty() && st == CUTENSOR_STATUS_SUCCESS) {
            const std::vector<Clip> box = todo.back().clips;
            const bool boxAcc = todo.back().acc;
            todo.pop_back();
            rs.clips = box;
            View v[3];
            Piece::Sub sub;
            for (int k = 0; k < 3; ++k) {
                v[k] = make_view(*T[k], *M[k], universe, radix, rs, !p.use[k].direct);
                sub.off[k] = v[k].offset;
                sub.hv[k].extent = v[k].extent; sub.hv[k].stride = v[k].stride; sub.hv[k].modes = v[k].modes;
            }
            if (p.subs.empty()) for (int k = 0; k < 3; ++k) p.use[k].off = v[k].offset;
            cutensorTensorDescriptor_t dT[3] = {nullptr, nullptr, nullptr};
            cutensorOperationDescriptor_t op = nullptr;
            cutensorPlanPreference_t pref = nullptr;
            for (int k = 0; k < 3 && st == CUTENSOR_STATUS_SUCCESS; ++k) st = make_desc(h, v[k], T[k]->dtype, &dT[k]);
            if (st == CUTENSOR_STATUS_SUCCESS)
                st = cutensorCreateContraction(h, &op, dT[0], v[0].modes.data(), CUTENSOR_OP_IDENTITY, dT[1], v[1].modes.data(), CUTENSOR_OP_IDENTITY,
                                               dT[2], v[2].modes.data(), CUTENSOR_OP_IDENTITY, dT[2], v[2].modes.data(), cd);
            if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlanPreference(h, &pref, CUTENSOR_ALGO_DEFAULT, CUTENSOR_JIT_MODE_NONE);
            if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlan(h, &sub.plan, op, pref, pl->contractionWs);
            if (st == CUTENSOR_STATUS_SUCCESS)
                st = cutensorPlanGetAttribute(h, sub.plan, CUTENSOR_PLAN_REQUIRED_WORKSPACE, &sub.ws, sizeof(sub.ws));
            cutensorDestroyOperationDescriptor(op);
            cutensorDestroyPlanPreference(pref);
            for (int k = 0; k < 3; ++k) cutensorDestroyTensorDescriptor(dT[k]);
            if (st != CUTENSOR_STATUS_SUCCESS) { cutensorDestroyPlan(sub.plan); break; }
            // Peeling: a local view with more than four unfusable modes in a group (block-cyclic (w, digit, digit...) splits of
            // several modes — blog_post.cu on 8 devices, scaling >= 2) would run on the functional mode-table kernel (measured
            // 650 GFLOP/s against 70,000+ for the tiled kernels).  Instead one block-index digit of the oversized group — the
            // one with the smallest extent — is taken out of the view and walked by the host: extent-many tiled contractions.
            int32_t grp[64], lab[64];
            int64_t ext[64];
            const int nm = (p.subs.size() + todo.size() < 512) ? ctamdPlanModeTableGroups(sub.plan, grp, lab, ext, 64) : 0;
            if (nm > 0 && !CTAMD_HOOK_IS("CUTENSORMG_AMD_PEEL", "0")) {
                int count[4] = {0, 0, 0, 0};
                for (int i = 0; i < std::min(nm, 64); ++i) ++count[grp[i]];
                int best = -1;
                for (int i = 0; i < std::min(nm, 64); ++i) {
                    if (count[grp[i]] <= 4 || (lab[i] & 7) == 7 || ext[i] < 2) continue;        // only digits (not w) of an oversized group
                    if (es == 2 && grp[i] == 3) continue;                                     // 16-bit data: never accumulate through D
                    if (best < 0 || ext[i] < ext[best]) best = i;
                }
                if (best >= 0) {
                    const int li = lab[best] >> 3, dj = lab[best] & 7;
                    std::vector<Clip> base = box;
                    Clip* c = nullptr;
                    for (Clip& x : base) if (x.label == li) c = &x;
                    if (c == nullptr) {        // first restriction of this label: everything it had in the view
                        Clip fresh;
                        fresh.label = li;
                        fresh.wHi = radix[(size_t)li].blockSize;
                        for (size_t j = 0; j < radix[(size_t)li].f.size(); ++j) fresh.digit.push_back({0, radix[(size_t)li].f[j]});
                        if (li == rs.qLabel && rs.qDigit >= 0) fresh.digit[(size_t)rs.qDigit] = {rs.c0, rs.c1};   // the piece's run of q's coordinate
                        base.push_back(fresh);
                        c = &base.back();
                    }
                    const std::pair<int64_t, int64_t> range = c->digit[(size_t)dj];
                    if (!rs.is_p(li) && range.second - range.first >= 2) {
                        cutensorDestroyPlan(sub.plan);
                        const bool contractedDigit = find_label(d.mC, universe[(size_t)li]) < 0;
                        for (int64_t val = range.second - 1; val >= range.first; --val) {      // pushed in reverse: executed in ascending order
                            c->digit[(size_t)dj] = {val, val + 1};
                            todo.push_back(Work{base, boxAcc || (contractedDigit && val > range.first)});
                        }
                        ++pl->peeled;
                        continue;
                    }
                }
            }
            sub.accumulate = boxAcc;
            p.subs.push_back(sub);
        }
        rs.clips.clear();
        if (st != CUTENSOR_STATUS_SUCCESS) break;
        if (p.use[2].direct) continue;
        // scatter plans: the piece's region inside every cell of C it touches (cell-relative strides)
        const View cellView = make_view(d.C, d.mC, universe, radix, rs, false);
        for (int c : p.use[2].cells) {
            cutensorTensorDescriptor_t ds = nullptr;
            cutensorOperationDescriptor_t po = nullptr;
            Piece::Scatter sc{c, cellView.offset, nullptr, {}};
            sc.hv.extent = cellView.extent; sc.hv.stride = cellView.stride; sc.hv.modes = cellView.modes;
            st = make_desc(h, cellView, d.C.dtype, &ds);
            if (st == CUTENSOR_STATUS_SUCCESS)
                st = cutensorCreatePermutation(h, &po, ds, cellView.modes.data(), CUTENSOR_OP_IDENTITY, ds, cellView.modes.data(), cd);
            if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlan(h, &sc.plan, po, nullptr, 0);
            cutensorDestroyOperationDescriptor(po);
            cutensorDestroyTensorDescriptor(ds);
            if (st != CUTENSOR_STATUS_SUCCESS) break;
            p.scatter.push_back(sc);
        }
        if (st != CUTENSOR_STATUS_SUCCESS) break;
    }
    if (st != CUTENSOR_STATUS_SUCCESS) {
        destroy_pieces(pieces);
        delete pl;
        return st;
    }
    // who stores into whose cells of D from afar (the owners' caller streams must end behind those stores)
    pl->scatterOwners.assign((size_t)(nDev * kComputeStreams), {});
    for (const Piece& p : pieces)
        for (const Piece::Scatter& sc : p.scatter) {
            std::vector<int>& v = pl->scatterOwners[(size_t)(p.dev * kComputeStreams + p.stream)];
            for (int o = 0; o < nDev; ++o)
                if (o != p.dev && handle->devices[(size_t)o] == d.C.devices[(size_t)sc.cell] && std::find(v.begin(), v.end(), o) == v.end())
                    v.push_back(o);
        }
    pl->pieces.swap(pieces);
    *plan = pl;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

cutensorStatus_t cutensorMgDestroyContractionPlan(cutensorMgContractionPlan_t plan) try {
    if (plan == nullptr) return CUTENSOR_STATUS_SUCCESS;
    destroy_pieces(plan->pieces);
    if (plan->owner != nullptr && plan->owner->haveDevice && plan->trialEv[0] != nullptr) {
        DeviceGuard guard;
        (void)hipSetDevice(plan->owner->devices[0]);
        for (hipEvent_t e : plan->trialEv) if (e) (void)hipEventDestroy(e);
    }
    if (!plan->events.empty() && plan->owner != nullptr) {
        DeviceGuard guard;
        const int nDev = (int)plan->owner->devices.size();
        for (int g = 0; g < nDev; ++g) {
            (void)hipSetDevice(plan->owner->devices[g]);
            for (int i = 0; i < plan->evPerDevice; ++i)
                if (plan->events[(size_t)(g * plan->evPerDevice + i)]) (void)hipEventDestroy(plan->events[(size_t)(g * plan->evPerDevice + i)]);
        }
    }
    delete plan;
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// Streams and events of the execution engine (created on first use; the Mg model is one host thread).
static bool ensure_runtime(cutensorMgHandle* h, cutensorMgContractionPlan* pl) {
    const int nDev = (int)h->devices.size();
    if (h->commStreams.size() != (size_t)nDev) { h->commStreams.assign((size_t)nDev, {}); h->auxStreams.assign((size_t)nDev, nullptr); }
    for (int g = 0; g < nDev; ++g) {
        if (hipSetDevice(h->devices[g]) != hipSuccess) return false;
        while ((int)h->commStreams[(size_t)g].size() < pl->commPerDevice) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return false;
            h->commStreams[(size_t)g].push_back(s);
        }
        if (h->auxStreams[(size_t)g] == nullptr && hipStreamCreateWithFlags(&h->auxStreams[(size_t)g], hipStreamNonBlocking) != hipSuccess) return false;
    }
    if (pl->events.empty()) {
        pl->events.assign((size_t)(nDev * pl->evPerDevice), nullptr);
        for (int g = 0; g < nDev; ++g) {
            if (hipSetDevice(h->devices[g]) != hipSuccess) return false;
            for (int i = 0; i < pl->evPerDevice; ++i)
                if (hipEventCreateWithFlags(&pl->events[(size_t)(g * pl->evPerDevice + i)], hipEventDisableTiming) != hipSuccess) return false;
        }
    }
    return true;
}

// contraction_multi_gpu.cu:328-332
cutensorStatus_t cutensorMgContraction(const cutensorMgHandle_t handle, const cutensorMgContractionPlan_t plan,
                                       const void* alpha, const void* A[], const void* B[], const void* beta,
                                       const void* C[], void* D[], void* workspaceDevice[], void* workspaceHost,
                                       cudaStream_t streams[]) try {
    (void)workspaceHost;
    if (handle == nullptr) return CUTENSOR_STATUS_NOT_INITIALIZED;
    if (plan == nullptr || alpha == nullptr || beta == nullptr || A == nullptr || B == nullptr || D == nullptr ||
        workspaceDevice == nullptr || streams == nullptr)
        return CUTENSOR_STATUS_INVALID_VALUE;
    if (!handle->haveDevice) return CUTENSOR_STATUS_ARCH_MISMATCH;   // plan-only handle (no GPU visible)
    DeviceGuard guard;
    cutensorMgContractionPlan* pl = plan;
    const cutensorMgContractionDescriptor& d = pl->desc;
    const int nDev = (int)handle->devices.size();
    const size_t es = elem_size(d.A.dtype);
    const bool f64 = d.A.dtype == HIP_R_64F || d.compute == CUTENSOR_COMPUTE_64F;
    const double b = f64 ? *static_cast<const double*>(beta) : (double)*static_cast<const float*>(beta);
    if (b != 0.0 && C == nullptr) return CUTENSOR_STATUS_INVALID_VALUE;
    if (!ensure_runtime(handle, pl)) { (void)hipGetLastError(); return CUTENSOR_STATUS_EXECUTION_FAILED; }
    const MgTensor* T[3] = {&d.A, &d.B, &d.C};
    const void* const* src[3] = {A, B, C};

    auto staging = [&](int g, int k) -> char* {   // k = 3, 4: contraction workspace of compute stream 0, 1
        char* base = static_cast<char*>(workspaceDevice[g]);
        for (int j = 0; j < k && j < 3; ++j) base += pl->stagingBytes[j];
        if (k > 3) base += (size_t)(k - 3) * pl->contractionWs;
        return base;
    };
    auto ev = [&](int g, int i) { return pl->events[(size_t)(g * pl->evPerDevice + i)]; };   // 0 start, 1 localReady, 2 auxDone, 3.. commDone
    auto compute_stream = [&](int g, int s) { return s == 0 ? streams[g] : handle->auxStreams[(size_t)g]; };
#define MG_HIP(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return CUTENSOR_STATUS_EXECUTION_FAILED; } } while (0)

    // ---- 0. fork: the helper streams of every device start behind the caller's stream ------------------------
    bool anyComm = false;
    for (int g = 0; g < nDev; ++g) anyComm = anyComm || pl->usesComm[(size_t)g];
    for (int g = 0; g < nDev; ++g) {
        if (!anyComm && !pl->usesAux[(size_t)g]) continue;
        MG_HIP(hipSetDevice(handle->devices[g]));
        MG_HIP(hipEventRecord(ev(g, 0), streams[g]));
    }
    for (int g = 0; g < nDev; ++g) {      // helper streams a plan never uses are left alone (one device, no transfers: no fork at all)
        MG_HIP(hipSetDevice(handle->devices[g]));
        if (pl->usesAux[(size_t)g]) MG_HIP(hipStreamWaitEvent(handle->auxStreams[(size_t)g], ev(g, 0), 0));
        if (!pl->usesComm[(size_t)g]) continue;
        for (hipStream_t cs : handle->commStreams[(size_t)g]) {
            // Peer copies PULL the owners' cells: the communication stream goes behind the caller's stream of every device.  Under RCCL
            // every rank's own communication stream takes part in a transfer (the owner sends from ITS stream), so a stream only has to
            // follow its own device's caller stream — 8 waits per call instead of 64 at eight devices (round 6: host cost of the call)
            if (pl->useRccl) { MG_HIP(hipStreamWaitEvent(cs, ev(g, 0), 0)); continue; }
            for (int o = 0; o < nDev; ++o) MG_HIP(hipStreamWaitEvent(cs, ev(o, 0), 0));
        }
    }

    // ---- 1. gather ---------------------------------------------------------------------------------------------
    // local cells (same physical device): device copies on the caller's stream of the receiving device, then the auxiliary stream
    // joins behind them — per device, so worker g issues device g's (MgWorkers) while this thread goes on with the remote transfers
    const bool threaded = handle->workers.active();
    auto local_stage = [&](int g) -> cutensorStatus_t {
        // up to kMgCopyBatch cells per launch (mg_kernels.hip): a device copy per cell costs the issuing thread 2-3 us
        MgCopyBatch batch;
        for (const Transfer& t : pl->transfers) {
            if (t.dst != g || !t.local || (t.tensor == 2 && b == 0.0) || t.bytes <= 0) continue;
            batch.src[batch.n] = src[t.tensor][t.cell];
            batch.dst[batch.n] = staging(t.dst, t.tensor) + (size_t)t.cell * (size_t)t.bytes;
            batch.bytes[batch.n] = (uint64_t)t.bytes;
            if (++batch.n == kMgCopyBatch) { MG_HIP(mg_copy_cells(batch, streams[g])); batch.n = 0; }
        }
        MG_HIP(mg_copy_cells(batch, streams[g]));
        if (pl->usesAux[(size_t)g]) {
            MG_HIP(hipEventRecord(ev(g, 1), streams[g]));
            MG_HIP(hipStreamWaitEvent(handle->auxStreams[(size_t)g], ev(g, 1), 0));
        }
        return CUTENSOR_STATUS_SUCCESS;
    };
    // a call without remote cells has nothing for this thread to do in between: the workers run staging and pieces in ONE phase (below)
    const bool onePhase = threaded && pl->numWaves == 0 && !anyComm;
    const std::function<cutensorStatus_t(int)> localStageFn = local_stage;
    // (whatever leaves this function while a phase is in flight — an error return, an exception on its way to the ABI's catch — collects
    // the workers first: they run lambdas that live on this stack frame)
    std::unique_lock<std::mutex> callLock(handle->callMutex, std::defer_lock);
    if (threaded) callLock.lock();
    struct PhaseGuard { MgWorkers* w; ~PhaseGuard() { if (w != nullptr) (void)w->wait(); } } phaseGuard{threaded ? &handle->workers : nullptr};
    if (onePhase) { }
    else if (threaded) handle->workers.run(localStageFn);
    else
        for (int g = 0; g < nDev; ++g) {
            MG_HIP(hipSetDevice(handle->devices[g]));
            const cutensorStatus_t stl = local_stage(g);
            if (stl != CUTENSOR_STATUS_SUCCESS) return stl;
        }
    // (from here to the wait() below an early return must collect the workers first: MG_HIP_W)
#define MG_HIP_W(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); if (threaded) (void)handle->workers.wait(); return CUTENSOR_STATUS_EXECUTION_FAILED; } } while (0)
    // transport of this call: all-gather for the tensors that qualify, or send/recv pairs for everything
    bool useAllGather = false;
    int trial = -1;   // auto: 0 / 1 = this call is the timed all-gather / send-recv trial
    if (pl->useRccl && (pl->allGatherEligible[0] || pl->allGatherEligible[1])) {
        if (pl->transport == 1) useAllGather = true;
        else if (pl->transport == 2) useAllGather = false;
        else {
            if (pl->calls < 2) { trial = pl->calls; useAllGather = trial == 0; }
            else {
                if (pl->chosen == 0 && pl->trialEv[3] != nullptr && hipEventQuery(pl->trialEv[3]) == hipSuccess) {
                    (void)hipSetDevice(handle->devices[0]);
                    if (hipEventElapsedTime(&pl->trialMs[0], pl->trialEv[0], pl->trialEv[1]) == hipSuccess &&
                        hipEventElapsedTime(&pl->trialMs[1], pl->trialEv[2], pl->trialEv[3]) == hipSuccess)
                        pl->chosen = pl->trialMs[0] <= pl->trialMs[1] ? 1 : 2;
                    else { (void)hipGetLastError(); pl->chosen = 1; }
                }
                (void)hipGetLastError();
                useAllGather = pl->chosen != 2;   // undecided: the collective
            }
        }
    }
    if (trial >= 0 && pl->trialEv[2 * trial] == nullptr) {
        (void)hipSetDevice(handle->devices[0]);
        if (hipEventCreate(&pl->trialEv[2 * trial]) != hipSuccess || hipEventCreate(&pl->trialEv[2 * trial + 1]) != hipSuccess) { (void)hipGetLastError(); trial = -1; }
    }
    ++pl->calls;
    if (trial >= 0) { MG_HIP_W(hipSetDevice(handle->devices[0])); MG_HIP_W(hipEventRecord(pl->trialEv[2 * trial], handle->commStreams[0][0])); }
    // remote cells, wave by wave
    for (int w = 0; w < pl->numWaves; ++w) {
        bool grouped = false;
        cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
        std::set<int> touched;   // events to record after this wave
        if (w == 0 && useAllGather) {
            // one ncclAllGather per device and qualifying tensor inside the group: device g contributes its own cell (cell g)
            // and receives the image [cell 0][cell 1]... straight into its staging area
            for (int k = 0; k < 2 && st == CUTENSOR_STATUS_SUCCESS; ++k) {
                if (!pl->allGatherEligible[k]) continue;
                if (!grouped) { (void)ncclGroupStart(); grouped = true; }
                for (int g = 0; g < nDev; ++g) {
                    (void)hipSetDevice(handle->devices[g]);
                    if (ncclAllGather(src[k][g], staging(g, k), (size_t)T[k]->cellElems, nccl_type(T[k]->dtype), handle->comms[(size_t)g],
                                      handle->commStreams[(size_t)g][0]) != ncclSuccess) { st = CUTENSOR_STATUS_EXECUTION_FAILED; break; }
                }
                for (const Transfer& t : pl->transfers)
                    if (t.tensor == k && !t.local) touched.insert(t.event);
            }
        }
        for (const Transfer& t : pl->transfers) {
            if (st != CUTENSOR_STATUS_SUCCESS) break;
            if (t.local || t.wave != w || (t.tensor == 2 && b == 0.0)) continue;
            if (useAllGather && t.tensor < 2 && pl->allGatherEligible[t.tensor]) continue;   // arrived with the collective
            char* dst = staging(t.dst, t.tensor) + (size_t)t.cell * (size_t)t.bytes;
            const int slot = (t.event - (t.dst * pl->evPerDevice + 3 + pl->commPerDevice)) % (pl->useRccl ? 1 : pl->commPerDevice);
            if (pl->useRccl && t.src >= 0) {
                if (!grouped) { (void)ncclGroupStart(); grouped = true; }
                (void)hipSetDevice(t.ownerDevice);
                if (ncclSend(src[t.tensor][t.cell], (size_t)T[t.tensor]->cellElems, nccl_type(T[t.tensor]->dtype), t.dst,
                             handle->comms[(size_t)t.src], handle->commStreams[(size_t)t.src][0]) != ncclSuccess) { st = CUTENSOR_STATUS_EXECUTION_FAILED; break; }
                (void)hipSetDevice(handle->devices[t.dst]);
                if (ncclRecv(dst, (size_t)T[t.tensor]->cellElems, nccl_type(T[t.tensor]->dtype), t.src, handle->comms[(size_t)t.dst],
                             handle->commStreams[(size_t)t.dst][0]) != ncclSuccess) { st = CUTENSOR_STATUS_EXECUTION_FAILED; break; }
            } else {
                (void)hipSetDevice(handle->devices[t.dst]);
                if (hipMemcpyPeerAsync(dst, handle->devices[t.dst], src[t.tensor][t.cell], t.ownerDevice, (size_t)t.bytes,
                                       handle->commStreams[(size_t)t.dst][(size_t)slot]) != hipSuccess) { st = CUTENSOR_STATUS_EXECUTION_FAILED; break; }
            }
            touched.insert(t.event);
        }
        if (grouped && ncclGroupEnd() != ncclSuccess) st = CUTENSOR_STATUS_EXECUTION_FAILED;   // also closes the group on the error path
        if (st != CUTENSOR_STATUS_SUCCESS) { (void)hipGetLastError(); if (threaded) (void)handle->workers.wait(); return st; }
        for (int e : touched) {
            const int g = e / pl->evPerDevice;
            const int slot = (e - (g * pl->evPerDevice + 3 + pl->commPerDevice)) % (pl->useRccl ? 1 : pl->commPerDevice);
            MG_HIP_W(hipSetDevice(handle->devices[g]));
            MG_HIP_W(hipEventRecord(pl->events[(size_t)e], handle->commStreams[(size_t)g][(size_t)slot]));
        }
        if (w == 0 && trial >= 0) { MG_HIP_W(hipSetDevice(handle->devices[0])); MG_HIP_W(hipEventRecord(pl->trialEv[2 * trial + 1], handle->commStreams[0][0])); }
    }
    if (pl->numWaves == 0 && trial >= 0) { MG_HIP_W(hipSetDevice(handle->devices[0])); MG_HIP_W(hipEventRecord(pl->trialEv[2 * trial + 1], handle->commStreams[0][0])); }

    // ---- 2. local contractions, 3. scatter ----------------------------------------------------------------------
    if (threaded && !onePhase) {       // the workers' staging copies are queued: the pieces of a device follow them on the same worker
        const cutensorStatus_t stw = handle->workers.wait();
        if (stw != CUTENSOR_STATUS_SUCCESS) return stw;
    }
    const float onef = 1.f;
    const double oned = 1.0;
    const void* one = f64 ? static_cast<const void*>(&oned) : static_cast<const void*>(&onef);
    // the pieces of device g, in plan order: waits for the wave events (all recorded above, by this thread), local contractions, scatters
    auto run_pieces = [&](int gWanted) -> cutensorStatus_t {
    std::set<std::pair<int, int>> waited;   // (device * 2 + stream, event): each stream waits for an event once
    for (const Piece& p : pl->pieces) {
        const int g = p.dev;
        if (gWanted >= 0 && g != gWanted) continue;
        if (gWanted < 0) MG_HIP(hipSetDevice(handle->devices[g]));
        hipStream_t cs = compute_stream(g, p.stream);
        for (int e : p.waitEvents) {
            if (b == 0.0) {   // events of waves that carried only C cells were never recorded
                bool live = false;
                for (const Transfer& t : pl->transfers) if (!t.local && t.event == e && t.tensor != 2) { live = true; break; }
                if (!live) continue;
            }
            if (waited.insert(std::make_pair(g * kComputeStreams + p.stream, e)).second) MG_HIP(hipStreamWaitEvent(cs, pl->events[(size_t)e], 0));
        }
        const char* pa = p.use[0].direct ? static_cast<const char*>(A[p.use[0].cell]) : staging(g, 0);
        const char* pb = p.use[1].direct ? static_cast<const char*>(B[p.use[1].cell]) : staging(g, 1);
        const char* pc;
        char* pd;
        if (p.use[2].direct) {
            pc = (b != 0.0) ? static_cast<const char*>(C[p.use[2].cell]) : static_cast<const char*>(D[p.use[2].cell]);
            pd = static_cast<char*>(D[p.use[2].cell]);
        } else {
            pc = staging(g, 2);
            pd = staging(g, 2);
        }
        cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
        for (size_t bi = 0; bi < p.subs.size(); ++bi) {   // boxes of the contracted index space accumulate into D
            const Piece::Sub& sub = p.subs[bi];
            const int64_t oC = sub.off[2] * (int64_t)es;
            st = cutensorContract(handle->handles[(size_t)g], sub.plan, alpha, pa + sub.off[0] * (int64_t)es, pb + sub.off[1] * (int64_t)es,
                                  sub.accumulate ? one : beta, (sub.accumulate ? pd : pc) + oC, pd + oC, staging(g, 3 + p.stream), pl->contractionWs, cs);
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
        }
        const size_t cellBytes = (size_t)d.C.cellElems * es;
        for (const Piece::Scatter& s : p.scatter) {
            const char* from = staging(g, 2) + (size_t)s.cell * cellBytes + s.off * (int64_t)es;
            char* to = static_cast<char*>(D[s.cell]) + s.off * (int64_t)es;
            st = cutensorPermute(handle->handles[(size_t)g], s.plan, one, from, to, cs);
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
        }
    }
    // the device's own join: its caller's stream ends behind its auxiliary and communication streams (every transfer of this call was
    // queued on them before the pieces started)
    for (int g = (gWanted >= 0 ? gWanted : 0); g < (gWanted >= 0 ? gWanted + 1 : nDev); ++g) {
        if (gWanted < 0) MG_HIP(hipSetDevice(handle->devices[g]));
        if (pl->usesAux[(size_t)g]) {
            MG_HIP(hipEventRecord(ev(g, 2), handle->auxStreams[(size_t)g]));
            MG_HIP(hipStreamWaitEvent(streams[g], ev(g, 2), 0));
        }
        for (size_t k = 0; pl->usesComm[(size_t)g] && k < handle->commStreams[(size_t)g].size() && (int)k < pl->commPerDevice; ++k) {
            MG_HIP(hipEventRecord(ev(g, 3 + (int)k), handle->commStreams[(size_t)g][k]));
            MG_HIP(hipStreamWaitEvent(streams[g], ev(g, 3 + (int)k), 0));
        }
    }
    // ... and the events the OTHER devices' caller streams wait for in step 4: the end of each compute stream that stored into cells of D
    // another handle device owns
    for (int g = (gWanted >= 0 ? gWanted : 0); g < (gWanted >= 0 ? gWanted + 1 : nDev); ++g)
        for (int sidx = 0; sidx < kComputeStreams; ++sidx) {
            if (pl->scatterOwners[(size_t)(g * kComputeStreams + sidx)].empty()) continue;
            if (gWanted < 0) MG_HIP(hipSetDevice(handle->devices[g]));
            MG_HIP(hipEventRecord(ev(g, pl->evScatter + sidx), compute_stream(g, sidx)));
        }
    return CUTENSOR_STATUS_SUCCESS;
    };
    {
        const std::function<cutensorStatus_t(int)> piecesFn = run_pieces;
        const std::function<cutensorStatus_t(int)> bothFn = [&](int g) -> cutensorStatus_t {
            const cutensorStatus_t s1 = local_stage(g);
            return s1 != CUTENSOR_STATUS_SUCCESS ? s1 : run_pieces(g);
        };
        cutensorStatus_t stp;
        if (threaded) { handle->workers.run(onePhase ? bothFn : piecesFn); stp = handle->workers.wait(); }
        else stp = run_pieces(-1);
        if (stp != CUTENSOR_STATUS_SUCCESS) return stp;
    }

    // ---- 4. join: the caller's stream of every device ends behind its helper streams (the device's own part ran with its pieces, above)
    //         — and behind every OTHER device's stream that stored into its cells of D (remote scatter) or still reads its cells of
    //         A / B / C (peer copies; under RCCL the owner's own communication stream takes part in the transfer and is joined there):
    //         a caller that synchronises only streams[owner], or chains a second call on it, sees finished cells.  All events were
    //         recorded by now; the waits of owner o only touch o's caller stream, so worker o issues them.
    bool anyCross = false;
    for (int g = 0; g < nDev && !anyCross; ++g) {
        for (int sidx = 0; sidx < kComputeStreams; ++sidx) anyCross = anyCross || !pl->scatterOwners[(size_t)(g * kComputeStreams + sidx)].empty();
        anyCross = anyCross || (!pl->useRccl && pl->usesComm[(size_t)g] && !pl->readOwners[(size_t)g].empty());
    }
    auto cross_join = [&](int oWanted) -> cutensorStatus_t {
        for (int g = 0; g < nDev; ++g) {
            for (int sidx = 0; sidx < kComputeStreams; ++sidx)
                for (int o : pl->scatterOwners[(size_t)(g * kComputeStreams + sidx)]) {
                    if (oWanted >= 0 && o != oWanted) continue;
                    if (oWanted < 0) MG_HIP(hipSetDevice(handle->devices[o]));
                    MG_HIP(hipStreamWaitEvent(streams[o], ev(g, pl->evScatter + sidx), 0));
                }
            if (pl->useRccl || !pl->usesComm[(size_t)g]) continue;
            for (size_t k = 0; k < handle->commStreams[(size_t)g].size() && (int)k < pl->commPerDevice; ++k)
                for (int o : pl->readOwners[(size_t)g]) {
                    if (oWanted >= 0 && o != oWanted) continue;
                    if (oWanted < 0) MG_HIP(hipSetDevice(handle->devices[o]));
                    MG_HIP(hipStreamWaitEvent(streams[o], ev(g, 3 + (int)k), 0));
                }
        }
        return CUTENSOR_STATUS_SUCCESS;
    };
    if (anyCross) {
        const std::function<cutensorStatus_t(int)> joinFn = cross_join;
        cutensorStatus_t stj;
        if (threaded) { handle->workers.run(joinFn); stj = handle->workers.wait(); }
        else stj = cross_join(-1);
        if (stj != CUTENSOR_STATUS_SUCCESS) return stj;
    }
#undef MG_HIP
#undef MG_HIP_W
    return CUTENSOR_STATUS_SUCCESS;
} CTAMD_API_CATCH

// ---- diagnostics (not part of the cuTENSORMg ABI; used by the tests and the bench) -------------------------------
// The boxes kbox_list() cuts the valid part [0, extent) of a padded index space into (block size, digit extents least
// significant first), as JSON: [{"wHi":..,"digits":[[lo,hi],...]},...].
int ctamdMgDescribeKBoxes(int64_t extent, int64_t blockSize, int nDigits, const int64_t* f, char* buf, size_t len) try {
    if (buf == nullptr || len == 0 || blockSize <= 0 || extent <= 0 || nDigits < 0 || (nDigits > 0 && f == nullptr)) return -1;
    Radix r;
    r.blockSize = blockSize;
    r.numBlocks = 1;
    for (int j = 0; j < nDigits; ++j) { r.f.push_back(f[j]); r.numBlocks *= f[j]; }
    if (extent > r.blockSize * r.numBlocks) return -1;
    std::string s = "[";
    char tmp[96];
    const std::vector<Clip> boxes = kbox_list(0, r, extent);
    for (size_t i = 0; i < boxes.size(); ++i) {
        std::snprintf(tmp, sizeof(tmp), "%s{\"wHi\":%lld,\"digits\":[", i ? "," : "", (long long)boxes[i].wHi);
        s += tmp;
        for (size_t j = 0; j < boxes[i].digit.size(); ++j) {
            std::snprintf(tmp, sizeof(tmp), "%s[%lld,%lld]", j ? "," : "", (long long)boxes[i].digit[j].first, (long long)boxes[i].digit[j].second);
            s += tmp;
        }
        s += "]}";
    }
    s += "]";
    if (s.size() + 1 > len) return -(int)(s.size() + 1);
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
} CTAMD_API_CATCH_INT


// ---------------------------------------------------------------------------------------------------------------------
// Host replay of a plan (test hook; not part of the cuTENSORMg ABI).  No multi-GPU box is reachable from the build container, so
// the N > 1 data path — which cells travel where, the [cell][cell buffer] staging images, the strided local views, the boxes of
// a ragged contracted mode, peeled digits, the scatter of staged C, and the events a piece waits for — is EXECUTED here over host
// memory instead of only being inspected: A / B / C / D are arrays of HOST cell buffers, every transfer is a memcpy into a host
// staging image, every local contraction is handed to `contract` (the caller's reference implementation: the tests pass the CPU
// oracle) on exactly the views, offsets, scalars and C / D aliasing cutensorMgContraction passes to cutensorContract, every
// scatter is a strided copy.  Staging images start as NaN.  Ordering is checked, not simulated: before a piece runs, every cell
// it reads from a staging image must have arrived by a local copy (caller's stream; the auxiliary stream starts behind them) or
// by a transfer whose event the piece's stream has waited for so far — a missing wait is an error even though the replay itself
// is sequential.  Returns 0, or a negative code with a message in `err`.
// ---------------------------------------------------------------------------------------------------------------------
#if CTAMD_HOOKS_BUILT     // compiled into the hooks flavour (lib_hooks/) only: the production library has no test entry points
typedef struct { int32_t n; const int64_t* extent; const int64_t* stride; const int32_t* modes; } ctamdMgHostView;
typedef int (*ctamdMgHostContractFn)(void* user, int dtype, const ctamdMgHostView* A, const void* a, const ctamdMgHostView* B, const void* b,
                                     const ctamdMgHostView* C, const void* c, void* d, double alpha, double beta);

int ctamdMgReplayOnHost(const cutensorMgContractionPlan_t plan, double alpha, const void* const A[], const void* const B[], double beta,
                        const void* const C[], void* const D[], ctamdMgHostContractFn contract, void* user, char* err, size_t errLen) try {
    auto fail = [&](int code, const std::string& msg) {
        if (err != nullptr && errLen > 0) { std::snprintf(err, errLen, "%s", msg.c_str()); }
        return code;
    };
    if (plan == nullptr || A == nullptr || B == nullptr || D == nullptr || contract == nullptr) return fail(-1, "invalid arguments");
    const cutensorMgContractionPlan* pl = plan;
    const cutensorMgContractionDescriptor& d = pl->desc;
    const int nDev = (int)pl->usesAux.size();
    const size_t es = elem_size(d.A.dtype);
    const void* const* src[3] = {A, B, C};
    if (beta != 0.0 && C == nullptr) return fail(-1, "beta != 0 without C");
    // staging images per device: NaN everywhere (an all-ones bit pattern is a NaN for fp16 / bf16 / fp32 / fp64)
    std::vector<std::vector<std::vector<char>>> stage((size_t)nDev, std::vector<std::vector<char>>(3));
    for (int g = 0; g < nDev; ++g)
        for (int k = 0; k < 3; ++k) stage[(size_t)g][(size_t)k].assign((size_t)pl->stagingBytes[k], (char)0xff);
    auto staging = [&](int g, int k) { return stage[(size_t)g][(size_t)k].data(); };
    // ---- 1. gather: every transfer the device path issues (same skip rule for C cells when beta == 0) ------------------------------
    std::map<std::pair<int, std::pair<int, int>>, int> arrivedBy;   // (device, (tensor, cell)) -> event, -1 = local copy
    for (const Transfer& t : pl->transfers) {
        if (t.tensor == 2 && beta == 0.0) continue;
        if ((size_t)(t.cell + 1) * (size_t)t.bytes > stage[(size_t)t.dst][(size_t)t.tensor].size())
            return fail(-2, "a transfer lands outside its staging image");
        if (src[t.tensor][t.cell] == nullptr) return fail(-1, "missing cell buffer");
        std::memcpy(staging(t.dst, t.tensor) + (size_t)t.cell * (size_t)t.bytes, src[t.tensor][t.cell], (size_t)t.bytes);
        arrivedBy[std::make_pair(t.dst, std::make_pair(t.tensor, t.cell))] = t.local ? -1 : t.event;
    }
    // ---- 2. pieces in execution order ---------------------------------------------------------------------------------------------
    std::vector<std::set<int>> waited((size_t)(nDev * kComputeStreams));
    const bool dropWaits = CTAMD_HOOK_IS("CUTENSORMG_AMD_TEST_DROP_WAITS", "1");
    for (size_t pi = 0; pi < pl->pieces.size(); ++pi) {
        const Piece& p = pl->pieces[pi];
        const int g = p.dev;
        std::set<int>& w = waited[(size_t)(g * kComputeStreams + p.stream)];
        // fault injection lives HERE, in the checker, never in the plan a device would execute: with CUTENSORMG_AMD_TEST_DROP_WAITS=1 the
        // replay pretends the pieces wait for nothing (tests/test_mg_replay_cpu.py proves the ordering check live with it)
        if (!dropWaits)
            for (int e : p.waitEvents) w.insert(e);
        for (int k = 0; k < 3; ++k) {
            if (p.use[k].direct || (k == 2 && beta == 0.0)) continue;
            for (int c : p.use[k].cells) {
                auto it = arrivedBy.find(std::make_pair(g, std::make_pair(k, c)));
                if (it == arrivedBy.end()) return fail(-3, "piece " + std::to_string(pi) + " reads a cell nothing transferred (tensor " + std::to_string(k) + ", cell " + std::to_string(c) + ")");
                if (it->second >= 0 && w.count(it->second) == 0)
                    return fail(-4, "piece " + std::to_string(pi) + " reads tensor " + std::to_string(k) + " cell " + std::to_string(c) + " without having waited for event " + std::to_string(it->second));
            }
        }
        const char* pa = p.use[0].direct ? static_cast<const char*>(A[p.use[0].cell]) : staging(g, 0);
        const char* pb = p.use[1].direct ? static_cast<const char*>(B[p.use[1].cell]) : staging(g, 1);
        const char* pc;
        char* pd;
        if (p.use[2].direct) {
            pc = (beta != 0.0) ? static_cast<const char*>(C[p.use[2].cell]) : static_cast<const char*>(D[p.use[2].cell]);
            pd = static_cast<char*>(D[p.use[2].cell]);
        } else {
            pc = staging(g, 2);
            pd = staging(g, 2);
        }
        for (const Piece::Sub& sub : p.subs) {
            ctamdMgHostView hv[3];
            for (int k = 0; k < 3; ++k) hv[k] = ctamdMgHostView{(int32_t)sub.hv[k].extent.size(), sub.hv[k].extent.data(), sub.hv[k].stride.data(), sub.hv[k].modes.data()};
            const int64_t oC = sub.off[2] * (int64_t)es;
            const int rc = contract(user, (int)d.A.dtype, &hv[0], pa + sub.off[0] * (int64_t)es, &hv[1], pb + sub.off[1] * (int64_t)es, &hv[2],
                                    (sub.accumulate ? pd : pc) + oC, pd + oC, alpha, sub.accumulate ? 1.0 : beta);
            if (rc != 0) return fail(-5, "the contraction callback failed on piece " + std::to_string(pi));
        }
        // ---- 3. scatter: the piece's region of every staged C cell goes to the owner's cell (identity permutation on strided views)
        const size_t cellBytes = (size_t)d.C.cellElems * es;
        for (const Piece::Scatter& sc : p.scatter) {
            const char* from = staging(g, 2) + (size_t)sc.cell * cellBytes + sc.off * (int64_t)es;
            char* to = static_cast<char*>(D[sc.cell]) + sc.off * (int64_t)es;
            const size_t n = sc.hv.extent.size();
            std::vector<int64_t> idx(n, 0);
            for (;;) {
                int64_t o = 0;
                for (size_t i = 0; i < n; ++i) o += idx[i] * sc.hv.stride[i];
                std::memcpy(to + o * (int64_t)es, from + o * (int64_t)es, es);
                size_t i = 0;
                for (; i < n; ++i) {
                    if (++idx[i] < sc.hv.extent[i]) break;
                    idx[i] = 0;
                }
                if (i == n) break;
            }
        }
    }
    return 0;
} CTAMD_API_CATCH_INT
#endif   // CTAMD_HOOKS_BUILT

// One JSON object describing the plan: which mode is sharded, the pieces in execution order with the grid cells they
// read in place / from the staging image and the events they wait for, and every cell transfer.
int ctamdMgDescribePlan(const cutensorMgContractionPlan_t plan, char* buf, size_t len) try {
    if (plan == nullptr || buf == nullptr || len == 0) return -1;
    std::string s;
    char tmp[256];
    auto add = [&](const char* fmt, auto... a) { std::snprintf(tmp, sizeof(tmp), fmt, a...); s += tmp; };
    int64_t remote = 0, local = 0;
    for (const Transfer& t : plan->transfers) (t.local ? local : remote) += t.bytes;
    {
        size_t subs = 0, libPeeled = 0, modeTable = 0;
        for (const Piece& p : plan->pieces) {
            subs += p.subs.size();
            for (const Piece::Sub& sub : p.subs) {
                if (ctamdPlanPeelLaunches(sub.plan) > 0) ++libPeeled;
                if (ctamdPlanModeTableGroups(sub.plan, nullptr, nullptr, nullptr, 0) > 0) ++modeTable;
            }
        }
        // peeled: digits this plan walks itself; libraryPeeled: local contractions the single-GPU library peels (one tiled inner
        // plan launched per index combination); modeTable: local contractions left to the functional mode-table kernel
        add("{\"peeled\":%d,\"libraryPeeled\":%llu,\"modeTable\":%llu,\"localContractions\":%llu,", plan->peeled, (unsigned long long)libPeeled,
            (unsigned long long)modeTable, (unsigned long long)subs);
    }
    add("\"numBoxes\":%d,\"allGatherEligible\":[%d,%d],\"transport\":\"%s\",\"trialMs\":[%.4f,%.4f],\"chosen\":%d,", plan->numBoxes,
        (int)plan->allGatherEligible[0], (int)plan->allGatherEligible[1],
        !plan->useRccl ? "peer" : (plan->transport == 2 || !(plan->allGatherEligible[0] || plan->allGatherEligible[1])) ? "sendrecv"
                                  : plan->transport == 1 ? "allgather" : "auto(allgather|sendrecv)",
        plan->trialMs[0], plan->trialMs[1], plan->chosen);
    s += "\"scatterOwners\":[";
    for (size_t i = 0; i < plan->scatterOwners.size(); ++i) {
        add("%s[", i ? "," : "");
        for (size_t j = 0; j < plan->scatterOwners[i].size(); ++j) add("%s%d", j ? "," : "", plan->scatterOwners[i][j]);
        s += "]";
    }
    s += "],\"readOwners\":[";
    for (size_t i = 0; i < plan->readOwners.size(); ++i) {
        add("%s[", i ? "," : "");
        for (size_t j = 0; j < plan->readOwners[i].size(); ++j) add("%s%d", j ? "," : "", plan->readOwners[i][j]);
        s += "]";
    }
    s += "],";
    add("\"p2Label\":%d,\"forceGather\":%d,", plan->p2Label, (int)plan->forceGather);
    add("\"pLabel\":%d,\"qLabel\":%d,\"numWaves\":%d,\"useRccl\":%d,\"commStreams\":%d,\"contractionWs\":%llu,", plan->pLabel, plan->qLabel,
        plan->numWaves, (int)plan->useRccl, plan->commPerDevice, (unsigned long long)plan->contractionWs);
    add("\"stagingBytes\":[%lld,%lld,%lld],\"remoteBytes\":%lld,\"localCopyBytes\":%lld,\"pieces\":[", (long long)plan->stagingBytes[0],
        (long long)plan->stagingBytes[1], (long long)plan->stagingBytes[2], (long long)remote, (long long)local);
    for (size_t i = 0; i < plan->pieces.size(); ++i) {
        const Piece& p = plan->pieces[i];
        add("%s{\"dev\":%d,\"lo\":%lld,\"hi\":%lld,\"lo2\":%lld,\"hi2\":%lld,\"q0\":%lld,\"q1\":%lld,\"stream\":%d,\"flops\":%.6g,\"use\":[", i ? "," : "", p.dev,
            (long long)p.lo, (long long)p.hi, (long long)p.lo2, (long long)p.hi2, (long long)p.q0, (long long)p.q1, p.stream, p.flops);
        for (int k = 0; k < 3; ++k) {
            add("%s{\"direct\":%d,\"off\":%lld,\"cells\":[", k ? "," : "", (int)p.use[k].direct, (long long)p.use[k].off);
            for (size_t c = 0; c < p.use[k].cells.size(); ++c) add("%s%d", c ? "," : "", p.use[k].cells[c]);
            s += "]}";
        }
        s += "],\"wait\":[";
        for (size_t e = 0; e < p.waitEvents.size(); ++e) add("%s%d", e ? "," : "", p.waitEvents[e]);
        s += "],\"scatter\":[";
        for (size_t c = 0; c < p.scatter.size(); ++c) add("%s%d", c ? "," : "", p.scatter[c].cell);
        s += "]}";
    }
    s += "],\"transfers\":[";
    for (size_t i = 0; i < plan->transfers.size(); ++i) {
        const Transfer& t = plan->transfers[i];
        add("%s{\"tensor\":%d,\"cell\":%d,\"dst\":%d,\"src\":%d,\"local\":%d,\"wave\":%d,\"bytes\":%lld,\"event\":%d}", i ? "," : "", t.tensor,
            t.cell, t.dst, t.src, (int)t.local, t.wave, (long long)t.bytes, t.event);
    }
    s += "]}";
    if (s.size() + 1 > len) return -(int)(s.size() + 1);
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
} CTAMD_API_CATCH_INT

}  // extern "C"

// =====================================================================================================================================
// cutensorMgCopy: dst[modesDst] = src[modesSrc] between two block-cyclic layouts (any block sizes, grids, ragged extents and
// strides on either side).  The contraction above does not use it: its scatter of staged C pieces is still the host loop of identity
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
