// mg_internal.hpp — what the translation units of libcutensorMg.so share: the layout and plan structs, the handle / descriptor / plan
// types behind cutensorMg.h's opaque pointers, the event-block layout, and the steps of the contraction plan builder
// (mg_contraction_plan.cpp) and of a contraction call (mg_contraction_exec.cpp).  The algorithm is described at the top of mg.cpp.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cutensor.h>
#include <cutensorMg.h>

#include "../host/api_guard.hpp"
#include "mg_workers.h"

// internal to libcutensorMg.so: the library exports its C entry points only
#define CTAMD_MG_HIDDEN __attribute__((visibility("hidden")))

extern "C" int ctamdLogLevel(void);   // libcutensor.so: CUTENSOR_LOG_LEVEL
extern "C" int ctamdPlanPeelLaunches(const cutensorPlan_t plan);
extern "C" int ctamdPlanModeTableGroups(const cutensorPlan_t plan, int32_t* group, int32_t* label, int64_t* extent, int maxOut);   // libcutensor.so diagnostic

namespace ctamd_mg CTAMD_MG_HIDDEN {

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

inline size_t elem_size(hipDataType t) {
    switch (t) {
        case HIP_R_16F: case HIP_R_16BF: return 2;
        case HIP_R_32F: return 4;
        case HIP_R_64F: return 8;
        default: return 0;
    }
}

constexpr int kMaxDigits = 6;      // block-index digits per label (labels of the local views: 8 * label + digit, 7 = w)
constexpr int kComputeStreams = 2; // caller's stream + one auxiliary stream per device
constexpr uint64_t kLocalContractionWs = 128ull << 20;   // split-K scratch offered to every local plan (per compute stream)

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
// A cell of C is gathered only to be scaled by beta: with beta == 0 its transfer is skipped — by the call's local staging copies, by
// its gather waves and by the host replay alike (and a wave event that would carry nothing else is never recorded: liveAtBetaZero).
inline bool skipped_at_beta_zero(const Transfer& t, bool betaIsZero) { return t.tensor == 2 && betaIsZero; }

// The events of a plan: one block per handle device,
//   0 start, 1 localReady, 2 auxDone, 3.. commDone[k] (one per communication stream), then one per (wave, slot) — a single slot under
//   RCCL (one event per device and wave), one per communication stream with peer copies —, then scatterDone[s] per compute stream.
// An "event" everywhere else is an index into the plan's event table, as these accessors return it.
struct EventLayout {
    int commPerDevice = 1, numWaves = 0, slotsPerWave = 1;
    EventLayout() = default;
    EventLayout(int commStreams, int waves, bool useRccl) : commPerDevice(commStreams), numWaves(waves), slotsPerWave(useRccl ? 1 : commStreams) {}
    int wave_base() const { return 3 + commPerDevice; }
    int scatter_base() const { return wave_base() + numWaves * slotsPerWave; }   // "evScatter" of the description
    int perDevice() const { return scatter_base() + kComputeStreams; }
    int start(int g) const { return g * perDevice(); }
    int localReady(int g) const { return g * perDevice() + 1; }
    int auxDone(int g) const { return g * perDevice() + 2; }
    int commDone(int g, int k) const { return g * perDevice() + 3 + k; }
    int wave(int g, int w, int slot) const { return g * perDevice() + wave_base() + w * slotsPerWave + slot; }
    int scatterDone(int g, int s) const { return g * perDevice() + scatter_base() + s; }
    int device_of(int event) const { return event / perDevice(); }
    int slot_of(int event) const { return (event % perDevice() - wave_base()) % slotsPerWave; }   // of a wave event: its communication stream
};

}  // namespace ctamd_mg

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
struct cutensorMgTensorDescriptor { ctamd_mg::MgTensor t; };
struct cutensorMgContractionDescriptor {
    ctamd_mg::MgTensor A, B, C, D;
    std::vector<int32_t> mA, mB, mC;
    cutensorComputeType_t compute;
};
struct cutensorMgContractionFind { cutensorMgAlgo_t algo; };
struct cutensorMgContractionPlan {
    cutensorMgContractionDescriptor desc;
    std::vector<ctamd_mg::Piece> pieces;       // execution order per device
    std::vector<ctamd_mg::Transfer> transfers;
    int64_t stagingBytes[3] = {0, 0, 0};
    uint64_t contractionWs = 0;                // per compute stream
    int pLabel = -1, qLabel = -1;
    int p2Label = -1;                          // second sharded mode (p shorter than 16 x devices), -1: none
    int numBoxes = 1;                          // local contractions per piece (> 1: a contracted mode is ragged)
    int peeled = 0;                            // how many times a digit of an oversized mode group was peeled into a host loop
    bool useRccl = false;
    bool forceGather = false;     // handle created under CUTENSORMG_AMD_FORCE_GATHER=1: operands always staged through the communication path
    ctamd_mg::EventLayout ev;                  // communication streams per device, waves, and where each event sits
    std::vector<hipEvent_t> events;            // created on first execution: nDev blocks of ev.perDevice()
    std::vector<char> liveAtBetaZero;          // per event: a wave event that carries at least one operand cell (one of C cells only is never
                                               // recorded when beta == 0, so no piece waits for it then)
    std::vector<char> usesAux, usesComm;       // per handle device: does any piece run on the auxiliary stream / any cell arrive from afar
    // ---- cross-device ordering the caller's streams owe each other (filled by the plan) ----
    // scatterOwners[g * kComputeStreams + s]: handle devices whose cells of D the pieces on (g, s) store into from afar: their
    // caller streams end behind that compute stream.  readOwners[g]: handle devices whose cells device g's communication
    // streams read by peer copies: their caller streams end behind those reads (the owner may overwrite its operand next).
    std::vector<std::vector<int>> scatterOwners, readOwners;
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

namespace ctamd_mg CTAMD_MG_HIDDEN {

class DeviceGuard {   // the caller's current device is restored (contraction_multi_gpu.cu:320-346)
public:
    DeviceGuard() { if (hipGetDevice(&saved_) != hipSuccess) { saved_ = -1; (void)hipGetLastError(); } }
    ~DeviceGuard() { if (saved_ >= 0) (void)hipSetDevice(saved_); }
private:
    int saved_ = -1;
};

inline int find_label(const std::vector<int32_t>& v, int32_t l) {
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == l) return (int)i;
    return -1;
}

inline int device_rank(const cutensorMgHandle* h, int32_t dev) {
    for (size_t i = 0; i < h->devices.size(); ++i)
        if (h->devices[i] == dev) return (int)i;
    return -1;
}

inline bool env_is(const char* name, const char* value) {
    const char* e = std::getenv(name);
    return e != nullptr && std::strcmp(e, value) == 0;
}
// test / measurement switches: read by the hooks flavour only (host/api_guard.hpp)
#if CTAMD_HOOKS_BUILT
#define CTAMD_HOOK_IS(NAME, VALUE) ::ctamd_mg::env_is(NAME, VALUE)
#else
#define CTAMD_HOOK_IS(NAME, VALUE) false
#endif

// The three operands of a contraction descriptor as tables: 0 = A, 1 = B, 2 = C / D.
struct Operands {
    const MgTensor* T[3];
    const std::vector<int32_t>* M[3];
    explicit Operands(const cutensorMgContractionDescriptor& d) : T{&d.A, &d.B, &d.C}, M{&d.mA, &d.mB, &d.mC} {}
};

// ---- index arithmetic of the views (mg_views.cpp; no HIP call) -------------------------------------------------------------------
struct View {
    std::vector<int64_t> extent, stride;
    std::vector<int32_t> modes;
    int64_t offset = 0;
};

// Clip of a (contracted, ragged) label to one box of its valid index space: w in [0, wHi), digit j in [lo_j, hi_j).
struct Clip {
    int label = -1;
    int64_t wHi = 0;
    std::vector<std::pair<int64_t, int64_t>> digit;
};
// Restriction of a label inside a view: the sharded mode p is pinned to [lo, hi) inside block `block`; q's digit
// `digit` is cut to [c0, c1).
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

std::vector<Clip> kbox_list(int li, const Radix& r, int64_t extent);
int grid_digits(const Radix& r, int64_t dc);
View make_view(const MgTensor& t, const std::vector<int32_t>& labels, const std::vector<int32_t>& universe,
               const std::vector<Radix>& radix, const Restrict& rs, bool staging);
std::vector<int> cells_of(const MgTensor& t, const std::vector<int32_t>& labels, const std::vector<int32_t>& universe,
                          const std::vector<Radix>& radix, const Restrict& rs);
uint32_t align_of(int64_t offsetBytes, size_t es);

// ---- the contraction plan builder (mg_contraction_plan.cpp), in the order cutensorMgCreateContractionPlan runs it -----------------
struct PlanInputs {               // what every step reads
    const cutensorMgHandle* h;
    const cutensorMgContractionDescriptor& d;     // the plan's own copy
    Operands ops;
    int nDev;
    size_t es;
    int wavesWanted;              // CUTENSORMG_AMD_WAVES
};
struct Labels { std::vector<int32_t> universe; std::vector<Radix> radix; };
struct Shard { int dev; int64_t lo, hi, lo2, hi2; };
struct Sharding {
    int pC = -1, pLi = -1;        // the sharded mode p: index in C, index in the label universe
    int p2C = -1, p2Li = -1;      // the second sharded mode
    int yK = -1;                  // the operand that does not carry p (gathered whole), -1: none
    int qLi = -1, qDigit = -1;    // the mode that orders the gather
    int64_t qCount = 1;
    std::vector<Shard> shards;
};
struct PlanDeleter { void operator()(cutensorMgContractionPlan* pl) const; };   // local plans, events, the plan itself
using PlanPtr = std::unique_ptr<cutensorMgContractionPlan, PlanDeleter>;
using Boxes = std::vector<std::vector<Clip>>;

void staging_sizes(const cutensorMgContractionDescriptor& d, int64_t out[3]);
int waves_wanted();
cutensorStatus_t build_radix(const PlanInputs& in, Labels* lab);
Sharding choose_sharding(const PlanInputs& in, const Labels& lab);
std::vector<Piece> cut_pieces(const PlanInputs& in, const Labels& lab, const Sharding& sh);
void plan_transfers(const PlanInputs& in, const Labels& lab, const Sharding& sh, cutensorMgContractionPlan* pl);
void classify_transport(const PlanInputs& in, cutensorMgContractionPlan* pl);
cutensorStatus_t contracted_boxes(const PlanInputs& in, const Labels& lab, Boxes* boxes);
cutensorStatus_t build_local_plans(const PlanInputs& in, const Labels& lab, const Sharding& sh, const Boxes& boxes, Piece& p, cutensorMgContractionPlan* pl);
cutensorStatus_t build_scatter_plans(const PlanInputs& in, const Labels& lab, const Sharding& sh, Piece& p);
void scatter_owners(const PlanInputs& in, cutensorMgContractionPlan* pl);

// ---- one piece, walked (the device call and the host replay execute a piece through this one function) ----------------------------
// Backend supplies
//   char* cell(int k, int c)                    the caller's buffer of cell c of A (k = 0), B (1), C (2), D (3)
//   char* staging(int g, int k)                 device g's staging image of tensor k
//   int contract(piece, sub, pa, pb, betaIsOne, pc, pd)     one local contraction: D = alpha A B + (betaIsOne ? 1 : beta) C
//   int scatter(piece, entry, from, to)         the piece's region of a staged C cell to the owner's cell
// and returns 0 or an error of its own, which ends the walk and is returned.
template <class Backend>
int walk_piece(const cutensorMgContractionPlan& pl, const Piece& p, bool betaIsZero, Backend& be) {
    const int64_t es = (int64_t)elem_size(pl.desc.A.dtype);
    const int g = p.dev;
    // operand bases: the cell itself (in place) or the device's staging image
    const char* pa = p.use[0].direct ? be.cell(0, p.use[0].cell) : be.staging(g, 0);
    const char* pb = p.use[1].direct ? be.cell(1, p.use[1].cell) : be.staging(g, 1);
    const char* pc;
    char* pd;
    if (p.use[2].direct) {
        pc = be.cell(betaIsZero ? 3 : 2, p.use[2].cell);     // beta == 0: C may be absent, D stands in (it is not read)
        pd = be.cell(3, p.use[2].cell);
    } else {
        pc = be.staging(g, 2);
        pd = be.staging(g, 2);
    }
    for (const Piece::Sub& sub : p.subs) {   // boxes of the contracted index space accumulate into D
        const int64_t oC = sub.off[2] * es;
        const int rc = be.contract(p, sub, pa + sub.off[0] * es, pb + sub.off[1] * es, sub.accumulate, (sub.accumulate ? pd : pc) + oC, pd + oC);
        if (rc != 0) return rc;
    }
    const size_t cellBytes = (size_t)pl.desc.C.cellElems * (size_t)es;
    for (const Piece::Scatter& s : p.scatter) {
        const char* from = be.staging(g, 2) + (size_t)s.cell * cellBytes + s.off * es;
        const int rc = be.scatter(p, s, from, be.cell(3, s.cell) + s.off * es);
        if (rc != 0) return rc;
    }
    return 0;
}

// ---- a contraction call (mg_contraction_exec.cpp) ---------------------------------------------------------------------------------
struct MgCall {                   // one cutensorMgContraction call: what every phase reads
    cutensorMgHandle* h;
    cutensorMgContractionPlan* pl;
    const void* alpha;
    const void* beta;
    const void* const* src[3];    // the caller's cell arrays of A, B, C
    void* const* D;
    void* const* workspace;
    hipStream_t* streams;
    int nDev;
    size_t es;
    bool f64;                     // the scalars are doubles
    double b;                     // beta
    bool betaIsZero;
    float onef = 1.f;
    double oned = 1.0;
    bool threaded = false, anyComm = false;

    MgCall(cutensorMgHandle* handle, cutensorMgContractionPlan* plan, const void* alpha_, const void* const* A, const void* const* B,
           const void* beta_, const void* const* C, void* const* D_, void* const* workspaceDevice, hipStream_t* streams_);
    const void* one() const { return f64 ? static_cast<const void*>(&oned) : static_cast<const void*>(&onef); }
    char* staging(int g, int k) const {            // device g's staging image of tensor k (k = 3: the end of the images)
        char* base = static_cast<char*>(workspace[g]);
        for (int j = 0; j < k && j < 3; ++j) base += pl->stagingBytes[j];
        return base;
    }
    char* contraction_ws(int g, int s) const { return staging(g, 3) + (size_t)s * pl->contractionWs; }   // of compute stream s
    hipEvent_t event(int e) const { return pl->events[(size_t)e]; }
    hipStream_t compute_stream(int g, int s) const { return s == 0 ? streams[g] : h->auxStreams[(size_t)g]; }
};
struct Transport { bool allGather = false; int trial = -1; };   // of one call; trial 0 / 1: the timed all-gather / send-recv call

bool ensure_runtime(cutensorMgHandle* h, cutensorMgContractionPlan* pl);
cutensorStatus_t fork(const MgCall& c);
cutensorStatus_t stage_local(const MgCall& c, int g);
cutensorStatus_t choose_transport(const MgCall& c, Transport* tr);
cutensorStatus_t gather_wave(const MgCall& c, int w, const Transport& tr);
cutensorStatus_t end_trial(const MgCall& c, const Transport& tr);
cutensorStatus_t run_pieces(const MgCall& c, int gWanted);      // gWanted < 0: every device, from the calling thread
cutensorStatus_t join_own(const MgCall& c, int gWanted);
bool any_cross_join(const MgCall& c);
cutensorStatus_t join_cross(const MgCall& c, int oWanted);

// The worker hand-off of a call (its rules: mg_contraction_exec.cpp).  A phase is a short list of steps; begin() hands it to the workers
// (worker g runs step(c, g) for each) and returns at once — collect() waits for them — or, on a handle without workers, runs
// step(c, -1) for each on the calling thread before it returns.
class WorkerPhases {
public:
    using Step = cutensorStatus_t (*)(const MgCall&, int);
    explicit WorkerPhases(const MgCall& c);
    ~WorkerPhases();
    WorkerPhases(const WorkerPhases&) = delete;
    WorkerPhases& operator=(const WorkerPhases&) = delete;
    cutensorStatus_t begin(std::initializer_list<Step> steps);      // at most three
    cutensorStatus_t collect();
    cutensorStatus_t run(std::initializer_list<Step> steps) {
        const cutensorStatus_t st = begin(steps);
        return st != CUTENSOR_STATUS_SUCCESS ? st : collect();
    }
private:
    const MgCall& c_;
    MgWorkers* workers_;
    std::unique_lock<std::mutex> lock_;
    MgWorkers::Phase fn_;
    Step steps_[3] = {nullptr, nullptr, nullptr};
    int nSteps_ = 0;
    bool inFlight_ = false;
};

}  // namespace ctamd_mg
