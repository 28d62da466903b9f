// mg_contraction_exec.cpp — the phases of a cutensorMgContraction call (mg.cpp runs them in order; steps 1-5 of the algorithm at the
// top of that file).  Every phase is a function over MgCall; a phase that takes a device index g >= 0 touches only that device's streams
// and is issued by worker g (which set its device once), with g < 0 it covers every device from the calling thread.
#include <set>

#include "mg_internal.hpp"
#include "mg_kernels.h"

namespace ctamd_mg {

#define MG_HIP(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return CUTENSOR_STATUS_EXECUTION_FAILED; } } while (0)

namespace {

ncclDataType_t nccl_type(hipDataType t) {
    switch (t) {
        case HIP_R_16F: return ncclFloat16;
        case HIP_R_16BF: return ncclBfloat16;
        case HIP_R_64F: return ncclFloat64;
        default: return ncclFloat32;
    }
}

// the devices a phase covers: g alone (a worker, its device is set) or all (the calling thread sets each)
struct DeviceRange {
    int first, last;
    bool setDevice;
    DeviceRange(const MgCall& c, int gWanted) : first(gWanted >= 0 ? gWanted : 0), last(gWanted >= 0 ? gWanted + 1 : c.nDev), setDevice(gWanted < 0) {}
};

}  // namespace

// Streams and events of the execution engine (created on first use; the Mg model is one host thread).
bool ensure_runtime(cutensorMgHandle* h, cutensorMgContractionPlan* pl) {
    const int nDev = (int)h->devices.size();
    if (h->commStreams.size() != (size_t)nDev) { h->commStreams.assign((size_t)nDev, {}); h->auxStreams.assign((size_t)nDev, nullptr); }
    for (int g = 0; g < nDev; ++g) {
        if (hipSetDevice(h->devices[g]) != hipSuccess) return false;
        while ((int)h->commStreams[(size_t)g].size() < pl->ev.commPerDevice) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return false;
            h->commStreams[(size_t)g].push_back(s);
        }
        if (h->auxStreams[(size_t)g] == nullptr && hipStreamCreateWithFlags(&h->auxStreams[(size_t)g], hipStreamNonBlocking) != hipSuccess) return false;
    }
    if (pl->events.empty()) {
        pl->events.assign((size_t)pl->ev.start(nDev), nullptr);
        for (int g = 0; g < nDev; ++g) {
            if (hipSetDevice(h->devices[g]) != hipSuccess) return false;
            for (int e = pl->ev.start(g); e < pl->ev.start(g + 1); ++e)
                if (hipEventCreateWithFlags(&pl->events[(size_t)e], hipEventDisableTiming) != hipSuccess) return false;
        }
    }
    return true;
}

MgCall::MgCall(cutensorMgHandle* handle, cutensorMgContractionPlan* plan, const void* alpha_, const void* const* A, const void* const* B,
               const void* beta_, const void* const* C, void* const* D_, void* const* workspaceDevice, hipStream_t* streams_)
    : h(handle), pl(plan), alpha(alpha_), beta(beta_), src{A, B, C}, D(D_), workspace(workspaceDevice), streams(streams_),
      nDev((int)handle->devices.size()), es(elem_size(plan->desc.A.dtype)),
      f64(plan->desc.A.dtype == HIP_R_64F || plan->desc.compute == CUTENSOR_COMPUTE_64F),
      b(f64 ? *static_cast<const double*>(beta_) : (double)*static_cast<const float*>(beta_)), betaIsZero(b == 0.0),
      threaded(handle->workers.active()) {
    for (int g = 0; g < nDev; ++g) anyComm = anyComm || plan->usesComm[(size_t)g];
}

// ---- 0. fork: the helper streams of every device start behind the caller's stream ------------------------
cutensorStatus_t fork(const MgCall& c) {
    const cutensorMgContractionPlan* pl = c.pl;
    for (int g = 0; g < c.nDev; ++g) {
        if (!c.anyComm && !pl->usesAux[(size_t)g]) continue;
        MG_HIP(hipSetDevice(c.h->devices[g]));
        MG_HIP(hipEventRecord(c.event(pl->ev.start(g)), c.streams[g]));
    }
    for (int g = 0; g < c.nDev; ++g) {      // helper streams a plan never uses are left alone (one device, no transfers: no fork at all)
        MG_HIP(hipSetDevice(c.h->devices[g]));
        if (pl->usesAux[(size_t)g]) MG_HIP(hipStreamWaitEvent(c.h->auxStreams[(size_t)g], c.event(pl->ev.start(g)), 0));
        if (!pl->usesComm[(size_t)g]) continue;
        for (hipStream_t cs : c.h->commStreams[(size_t)g]) {
            // Peer copies PULL the owners' cells: the communication stream goes behind the caller's stream of every device.  Under RCCL
            // every rank's own communication stream takes part in a transfer (the owner sends from ITS stream), so a stream only has to
            // follow its own device's caller stream — 8 waits per call instead of 64 at eight devices (round 6: host cost of the call)
            if (pl->useRccl) { MG_HIP(hipStreamWaitEvent(cs, c.event(pl->ev.start(g)), 0)); continue; }
            for (int o = 0; o < c.nDev; ++o) MG_HIP(hipStreamWaitEvent(cs, c.event(pl->ev.start(o)), 0));
        }
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- 1. gather, local cells (same physical device): device copies on the caller's stream of the receiving device, then the auxiliary
//         stream joins behind them
cutensorStatus_t stage_local(const MgCall& c, int gWanted) {
    const cutensorMgContractionPlan* pl = c.pl;
    const DeviceRange r(c, gWanted);
    for (int g = r.first; g < r.last; ++g) {
        if (r.setDevice) MG_HIP(hipSetDevice(c.h->devices[g]));
        // up to kMgCopyBatch cells per launch (mg_kernels.hip): a device copy per cell costs the issuing thread 2-3 us
        MgCopyBatch batch;
        for (const Transfer& t : pl->transfers) {
            if (t.dst != g || !t.local || skipped_at_beta_zero(t, c.betaIsZero) || t.bytes <= 0) continue;
            batch.src[batch.n] = c.src[t.tensor][t.cell];
            batch.dst[batch.n] = c.staging(t.dst, t.tensor) + (size_t)t.cell * (size_t)t.bytes;
            batch.bytes[batch.n] = (uint64_t)t.bytes;
            if (++batch.n == kMgCopyBatch) { MG_HIP(mg_copy_cells(batch, c.streams[g])); batch.n = 0; }
        }
        MG_HIP(mg_copy_cells(batch, c.streams[g]));
        if (pl->usesAux[(size_t)g]) {
            MG_HIP(hipEventRecord(c.event(pl->ev.localReady(g)), c.streams[g]));
            MG_HIP(hipStreamWaitEvent(c.h->auxStreams[(size_t)g], c.event(pl->ev.localReady(g)), 0));
        }
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- transport of this call: all-gather for the tensors that qualify, or send/recv pairs for everything.  auto: the first two calls
//      are the timed trials (their events on device 0's communication stream), later calls take the faster
cutensorStatus_t choose_transport(const MgCall& c, Transport* tr) {
    cutensorMgContractionPlan* pl = c.pl;
    tr->allGather = false;
    tr->trial = -1;
    if (pl->useRccl && (pl->allGatherEligible[0] || pl->allGatherEligible[1])) {
        if (pl->transport == 1) tr->allGather = true;
        else if (pl->transport == 2) tr->allGather = false;
        else if (pl->calls < 2) { tr->trial = pl->calls; tr->allGather = tr->trial == 0; }
        else {
            if (pl->chosen == 0 && pl->trialEv[3] != nullptr && hipEventQuery(pl->trialEv[3]) == hipSuccess) {
                (void)hipSetDevice(c.h->devices[0]);
                if (hipEventElapsedTime(&pl->trialMs[0], pl->trialEv[0], pl->trialEv[1]) == hipSuccess &&
                    hipEventElapsedTime(&pl->trialMs[1], pl->trialEv[2], pl->trialEv[3]) == hipSuccess)
                    pl->chosen = pl->trialMs[0] <= pl->trialMs[1] ? 1 : 2;
                else { (void)hipGetLastError(); pl->chosen = 1; }
            }
            (void)hipGetLastError();
            tr->allGather = pl->chosen != 2;   // undecided: the collective
        }
    }
    if (tr->trial >= 0 && pl->trialEv[2 * tr->trial] == nullptr) {
        (void)hipSetDevice(c.h->devices[0]);
        if (hipEventCreate(&pl->trialEv[2 * tr->trial]) != hipSuccess || hipEventCreate(&pl->trialEv[2 * tr->trial + 1]) != hipSuccess) { (void)hipGetLastError(); tr->trial = -1; }
    }
    ++pl->calls;
    if (tr->trial >= 0) { MG_HIP(hipSetDevice(c.h->devices[0])); MG_HIP(hipEventRecord(pl->trialEv[2 * tr->trial], c.h->commStreams[0][0])); }
    return CUTENSOR_STATUS_SUCCESS;
}

cutensorStatus_t end_trial(const MgCall& c, const Transport& tr) {
    if (tr.trial < 0) return CUTENSOR_STATUS_SUCCESS;
    MG_HIP(hipSetDevice(c.h->devices[0]));
    MG_HIP(hipEventRecord(c.pl->trialEv[2 * tr.trial + 1], c.h->commStreams[0][0]));
    return CUTENSOR_STATUS_SUCCESS;
}

namespace {

// one ncclAllGather per device and qualifying tensor inside the group: device g contributes its own cell (cell g) and receives the
// image [cell 0][cell 1]... straight into its staging area
cutensorStatus_t all_gather(const MgCall& c, bool* grouped, std::set<int>* touched) {
    const cutensorMgContractionPlan* pl = c.pl;
    const Operands ops(pl->desc);
    for (int k = 0; k < 2; ++k) {
        if (!pl->allGatherEligible[k]) continue;
        if (!*grouped) { (void)ncclGroupStart(); *grouped = true; }
        for (int g = 0; g < c.nDev; ++g) {
            (void)hipSetDevice(c.h->devices[g]);
            if (ncclAllGather(c.src[k][g], c.staging(g, k), (size_t)ops.T[k]->cellElems, nccl_type(ops.T[k]->dtype), c.h->comms[(size_t)g],
                              c.h->commStreams[(size_t)g][0]) != ncclSuccess) return CUTENSOR_STATUS_EXECUTION_FAILED;
        }
        for (const Transfer& t : pl->transfers)
            if (t.tensor == k && !t.local) touched->insert(t.event);
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// one remote cell: an ncclSend / ncclRecv pair inside the wave's group, or a peer copy on the communication stream of its event
cutensorStatus_t transfer_cell(const MgCall& c, const Transfer& t, bool* grouped) {
    const cutensorMgContractionPlan* pl = c.pl;
    const MgTensor& T = *Operands(pl->desc).T[t.tensor];
    char* dst = c.staging(t.dst, t.tensor) + (size_t)t.cell * (size_t)t.bytes;
    if (pl->useRccl && t.src >= 0) {
        if (!*grouped) { (void)ncclGroupStart(); *grouped = true; }
        (void)hipSetDevice(t.ownerDevice);
        if (ncclSend(c.src[t.tensor][t.cell], (size_t)T.cellElems, nccl_type(T.dtype), t.dst, c.h->comms[(size_t)t.src],
                     c.h->commStreams[(size_t)t.src][0]) != ncclSuccess) return CUTENSOR_STATUS_EXECUTION_FAILED;
        (void)hipSetDevice(c.h->devices[t.dst]);
        if (ncclRecv(dst, (size_t)T.cellElems, nccl_type(T.dtype), t.src, c.h->comms[(size_t)t.dst],
                     c.h->commStreams[(size_t)t.dst][0]) != ncclSuccess) return CUTENSOR_STATUS_EXECUTION_FAILED;
    } else {
        (void)hipSetDevice(c.h->devices[t.dst]);
        if (hipMemcpyPeerAsync(dst, c.h->devices[t.dst], c.src[t.tensor][t.cell], t.ownerDevice, (size_t)t.bytes,
                               c.h->commStreams[(size_t)t.dst][(size_t)pl->ev.slot_of(t.event)]) != hipSuccess) return CUTENSOR_STATUS_EXECUTION_FAILED;
    }
    return CUTENSOR_STATUS_SUCCESS;
}

}  // namespace

// ---- 1. gather, remote cells of wave w: the transfers, then the wave's events on the communication streams that carried them -----------
cutensorStatus_t gather_wave(const MgCall& c, int w, const Transport& tr) {
    const cutensorMgContractionPlan* pl = c.pl;
    bool grouped = false;
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    std::set<int> touched;   // events to record after this wave
    if (w == 0 && tr.allGather) st = all_gather(c, &grouped, &touched);
    for (const Transfer& t : pl->transfers) {
        if (st != CUTENSOR_STATUS_SUCCESS) break;
        if (t.local || t.wave != w || skipped_at_beta_zero(t, c.betaIsZero)) continue;
        if (tr.allGather && t.tensor < 2 && pl->allGatherEligible[t.tensor]) continue;   // arrived with the collective
        st = transfer_cell(c, t, &grouped);
        if (st == CUTENSOR_STATUS_SUCCESS) touched.insert(t.event);
    }
    if (grouped && ncclGroupEnd() != ncclSuccess) st = CUTENSOR_STATUS_EXECUTION_FAILED;   // also closes the group on the error path
    if (st != CUTENSOR_STATUS_SUCCESS) { (void)hipGetLastError(); return st; }
    for (int e : touched) {
        const int g = pl->ev.device_of(e);
        MG_HIP(hipSetDevice(c.h->devices[g]));
        MG_HIP(hipEventRecord(c.event(e), c.h->commStreams[(size_t)g][(size_t)pl->ev.slot_of(e)]));
    }
    return w == 0 ? end_trial(c, tr) : CUTENSOR_STATUS_SUCCESS;
}

namespace {

// walk_piece on the device: the caller's cell buffers and the workspace, cutensorContract / cutensorPermute on the piece's stream
struct DeviceBackend {
    const MgCall& c;
    char* cell(int k, int cell) const { return k == 3 ? static_cast<char*>(c.D[cell]) : static_cast<char*>(const_cast<void*>(c.src[k][cell])); }
    char* staging(int g, int k) const { return c.staging(g, k); }
    int contract(const Piece& p, const Piece::Sub& sub, const char* pa, const char* pb, bool betaIsOne, const char* pc, char* pd) const {
        return (int)cutensorContract(c.h->handles[(size_t)p.dev], sub.plan, c.alpha, pa, pb, betaIsOne ? c.one() : c.beta, pc, pd,
                                     c.contraction_ws(p.dev, p.stream), c.pl->contractionWs, c.compute_stream(p.dev, p.stream));
    }
    int scatter(const Piece& p, const Piece::Scatter& s, const char* from, char* to) const {
        return (int)cutensorPermute(c.h->handles[(size_t)p.dev], s.plan, c.one(), from, to, c.compute_stream(p.dev, p.stream));
    }
};

}  // namespace

// ---- 2. local contractions, 3. scatter: the pieces of device g, in plan order — waits for the wave events (all recorded by the calling
//         thread before this phase), then the piece (walk_piece)
cutensorStatus_t run_pieces(const MgCall& c, int gWanted) {
    const cutensorMgContractionPlan* pl = c.pl;
    DeviceBackend backend{c};
    std::set<std::pair<int, int>> waited;   // (device * 2 + stream, event): each stream waits for an event once
    for (const Piece& p : pl->pieces) {
        const int g = p.dev;
        if (gWanted >= 0 && g != gWanted) continue;
        if (gWanted < 0) MG_HIP(hipSetDevice(c.h->devices[g]));
        hipStream_t cs = c.compute_stream(g, p.stream);
        for (int e : p.waitEvents) {
            if (c.betaIsZero && !pl->liveAtBetaZero[(size_t)e]) continue;   // events of waves that carried only C cells were never recorded
            if (waited.insert(std::make_pair(g * kComputeStreams + p.stream, e)).second) MG_HIP(hipStreamWaitEvent(cs, c.event(e), 0));
        }
        const int rc = walk_piece(*pl, p, c.betaIsZero, backend);
        if (rc != 0) return (cutensorStatus_t)rc;
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- 4. join, the device's own part: its caller's stream ends behind its auxiliary and communication streams (every transfer of this
//         call was queued on them before the pieces started) ... and the events the OTHER devices' caller streams wait for in
//         join_cross: the end of each compute stream that stored into cells of D another handle device owns
cutensorStatus_t join_own(const MgCall& c, int gWanted) {
    const cutensorMgContractionPlan* pl = c.pl;
    const DeviceRange r(c, gWanted);
    for (int g = r.first; g < r.last; ++g) {
        if (r.setDevice) MG_HIP(hipSetDevice(c.h->devices[g]));
        if (pl->usesAux[(size_t)g]) {
            MG_HIP(hipEventRecord(c.event(pl->ev.auxDone(g)), c.h->auxStreams[(size_t)g]));
            MG_HIP(hipStreamWaitEvent(c.streams[g], c.event(pl->ev.auxDone(g)), 0));
        }
        for (size_t k = 0; pl->usesComm[(size_t)g] && k < c.h->commStreams[(size_t)g].size() && (int)k < pl->ev.commPerDevice; ++k) {
            MG_HIP(hipEventRecord(c.event(pl->ev.commDone(g, (int)k)), c.h->commStreams[(size_t)g][k]));
            MG_HIP(hipStreamWaitEvent(c.streams[g], c.event(pl->ev.commDone(g, (int)k)), 0));
        }
    }
    for (int g = r.first; g < r.last; ++g)
        for (int sidx = 0; sidx < kComputeStreams; ++sidx) {
            if (pl->scatterOwners[(size_t)(g * kComputeStreams + sidx)].empty()) continue;
            if (r.setDevice) MG_HIP(hipSetDevice(c.h->devices[g]));
            MG_HIP(hipEventRecord(c.event(pl->ev.scatterDone(g, sidx)), c.compute_stream(g, sidx)));
        }
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- 4. join across devices: the caller's stream of every device also ends behind every OTHER device's stream that stored into its
//         cells of D (remote scatter) or still reads its cells of A / B / C (peer copies; under RCCL the owner's own communication
//         stream takes part in the transfer and is joined in join_own): a caller that synchronises only streams[owner], or chains a
//         second call on it, sees finished cells.  All events were recorded by now; the waits of owner o only touch o's caller stream,
//         so worker o issues them.
bool any_cross_join(const MgCall& c) {
    const cutensorMgContractionPlan* pl = c.pl;
    for (int g = 0; g < c.nDev; ++g) {
        for (int sidx = 0; sidx < kComputeStreams; ++sidx)
            if (!pl->scatterOwners[(size_t)(g * kComputeStreams + sidx)].empty()) return true;
        if (!pl->useRccl && pl->usesComm[(size_t)g] && !pl->readOwners[(size_t)g].empty()) return true;
    }
    return false;
}

cutensorStatus_t join_cross(const MgCall& c, int oWanted) {
    const cutensorMgContractionPlan* pl = c.pl;
    for (int g = 0; g < c.nDev; ++g) {
        for (int sidx = 0; sidx < kComputeStreams; ++sidx)
            for (int o : pl->scatterOwners[(size_t)(g * kComputeStreams + sidx)]) {
                if (oWanted >= 0 && o != oWanted) continue;
                if (oWanted < 0) MG_HIP(hipSetDevice(c.h->devices[o]));
                MG_HIP(hipStreamWaitEvent(c.streams[o], c.event(pl->ev.scatterDone(g, sidx)), 0));
            }
        if (pl->useRccl || !pl->usesComm[(size_t)g]) continue;
        for (size_t k = 0; k < c.h->commStreams[(size_t)g].size() && (int)k < pl->ev.commPerDevice; ++k)
            for (int o : pl->readOwners[(size_t)g]) {
                if (oWanted >= 0 && o != oWanted) continue;
                if (oWanted < 0) MG_HIP(hipSetDevice(c.h->devices[o]));
                MG_HIP(hipStreamWaitEvent(c.streams[o], c.event(pl->ev.commDone(g, (int)k)), 0));
            }
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- the worker hand-off ------------------------------------------------------------------------------------------------------------
// Its three rules are enforced here and nowhere else:
//   1. a phase's callable outlives the phase: it is the member fn_ (one for all phases of the call; the steps it runs are set before
//      every run()), and this object lives on the entry point's frame until the call returns;
//   2. every exit between run() and wait() collects the workers: the destructor waits for a phase still in flight, whatever leaves the
//      entry point — an error return, an exception on its way to the ABI's catch;
//   3. calls on one handle are serialised: the workers take one phase at a time, so callMutex is held for the lifetime of this object.
WorkerPhases::WorkerPhases(const MgCall& c) : c_(c), workers_(c.threaded ? &c.h->workers : nullptr) {
    if (workers_ == nullptr) return;
    lock_ = std::unique_lock<std::mutex>(c.h->callMutex);
    fn_ = [this](int g) -> int {
        try {
            for (int i = 0; i < nSteps_; ++i) {
                const cutensorStatus_t st = steps_[i](c_, g);
                if (st != CUTENSOR_STATUS_SUCCESS) return (int)st;
            }
            return 0;
        } catch (...) { return (int)CUTENSOR_STATUS_INTERNAL_ERROR; }
    };
}

WorkerPhases::~WorkerPhases() {
    if (inFlight_) (void)workers_->wait();
}

cutensorStatus_t WorkerPhases::begin(std::initializer_list<Step> steps) {
    nSteps_ = 0;
    for (Step s : steps) steps_[nSteps_++] = s;
    if (workers_ != nullptr) {
        workers_->run(fn_);
        inFlight_ = true;
        return CUTENSOR_STATUS_SUCCESS;
    }
    for (int i = 0; i < nSteps_; ++i) {
        const cutensorStatus_t st = steps_[i](c_, -1);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
    }
    return CUTENSOR_STATUS_SUCCESS;
}

cutensorStatus_t WorkerPhases::collect() {
    if (!inFlight_) return CUTENSOR_STATUS_SUCCESS;
    inFlight_ = false;
    return (cutensorStatus_t)workers_->wait();
}

#undef MG_HIP

}  // namespace ctamd_mg
