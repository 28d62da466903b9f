// mp_plan.cpp — the steps of cutensorMpCreatePlan (mp.cpp has the sequence): the boxes of C, the algorithm, then either transfers,
// staging and the local contraction of the gather algorithm, or the regions, copies and local contraction of the reduce algorithm.
// Every step derives its part from the descriptors alone, identically on every rank, and takes its workspace regions from one layout.
#include <cstring>

#include "mp_internal.hpp"

namespace ctamd_mp CTAMD_MP_HIDDEN {

cutensorStatus_t own_c_boxes(PlanContext& c) {
    const cutensorMpOperationDescriptor& d = c.pl.desc;
    c.cBox.resize((size_t)c.pl.nranks);
    for (int q = 0; q < c.pl.nranks; ++q) {
        const int64_t cell = cell_of_rank(d.C, q);
        if (cell < 0) return CUTENSOR_STATUS_INTERNAL_ERROR;
        c.cBox[(size_t)q] = cell_box(d.C, cell);
    }
    c.pl.compute = !c.cBox[(size_t)c.pl.rank].empty();
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- algorithm selection -----------------------------------------------------------------------------------------------
// Bytes every rank would receive under the gather algorithm, summed over ranks.
static int64_t gather_traffic(const cutensorMpOperationDescriptor& d, const std::vector<Box>& cBox, int world, int64_t es) {
    int64_t total = 0;
    for (int k = 0; k < 2; ++k) {
        const MpTensor& x = d.operand(k);
        if (x.replicated()) continue;
        for (int q = 0; q < world; ++q) {
            if (cBox[(size_t)q].empty()) continue;
            const Box need = needed_box(x, d.modes(k), d.mC, cBox[(size_t)q]);
            for (int64_t c = 0; c < x.numCells; ++c)
                if (x.owner[(size_t)c] != q) total += intersect(need, cell_box(x, c)).volume() * es;
        }
    }
    return total;
}

// The reduce algorithm applies when A and B are cut along contracted modes only and every rank holds the same
// non-empty K range of both.
static bool reduce_applicable(const cutensorMpOperationDescriptor& d, int world) {
    if (d.A.replicated() || d.B.replicated() || world < 2) return false;
    for (int k = 0; k < 2; ++k)
        for (uint32_t i = 0; i < d.operand(k).n; ++i) {
            if (d.operand(k).p[i] == 1) continue;
            if (find_label(d.mC, d.modes(k)[i]) >= 0) return false;            // a free / batch mode is cut
            if (find_label(d.modes(1 - k), d.modes(k)[i]) < 0) return false;
        }
    for (int r = 0; r < world; ++r) {
        const Box a = block_of_rank(d.A, r), b = block_of_rank(d.B, r);
        if (a.empty() || b.empty()) return false;
        for (uint32_t i = 0; i < d.A.n; ++i) {
            const int j = find_label(d.mB, d.mA[i]);
            if (j >= 0 && (a.lo[i] != b.lo[(size_t)j] || a.hi[i] != b.hi[(size_t)j])) return false;
        }
    }
    return true;
}

// Identical inputs on every rank, hence an identical choice: the byte counts, unless the test hook names the algorithm.
bool choose_algorithm(PlanContext& c) {
    cutensorMpPlan& pl = c.pl;
    const cutensorMpOperationDescriptor& d = pl.desc;
    const int64_t es = (int64_t)elem_size(d.A.dtype);
    pl.gatherTotal = gather_traffic(d, c.cBox, pl.nranks, es);
    // ring all-reduce moves ~2 |C| per rank, reduce-scatter ~|C|
    pl.reduceTotal = (int64_t)pl.nranks * whole_box(d.C.extent).volume() * es * (d.C.replicated() ? 2 : 1);
    bool useReduce = reduce_applicable(d, pl.nranks) && pl.reduceTotal < pl.gatherTotal;
    if (const char* force = CTAMD_HOOK_ENV("CUTENSORMP_AMD_ALGO")) {       // tests: "gather" / "reduce" on every rank
        if (std::strcmp(force, "gather") == 0) useReduce = false;
        else if (std::strcmp(force, "reduce") == 0) useReduce = reduce_applicable(d, pl.nranks);
    }
    return useReduce;
}

// ---- the local contraction, for both algorithms -------------------------------------------------------------------------------
cutensorStatus_t plan_local_contraction(PlanContext& c, const TensorView (&view)[3], uint64_t budget) {
    cutensorMpPlan& pl = c.pl;
    const cutensorMpOperationDescriptor& d = pl.desc;
    cutensorHandle_t h = c.handle->h;
    EngineTemps tmp;
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    for (int k = 0; k < 3 && st == CUTENSOR_STATUS_SUCCESS; ++k)
        st = cutensorCreateTensorDescriptor(h, &tmp.desc[k], d.operand(k).n, view[k].extent.data(), view[k].stride.data(), d.operand(k).dtype, view[k].align);
    if (st == CUTENSOR_STATUS_SUCCESS)
        st = cutensorCreateContraction(h, &tmp.op, tmp.desc[0], d.mA.data(), d.opA, tmp.desc[1], d.mB.data(), d.opB, tmp.desc[2], d.mC.data(), d.opC,
                                       tmp.desc[2], d.mC.data(), d.compute);
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlanPreference(h, &tmp.pref, CUTENSOR_ALGO_DEFAULT, CUTENSOR_JIT_MODE_NONE);
    uint64_t want = 0;
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorEstimateWorkspaceSize(h, tmp.op, tmp.pref, CUTENSOR_WORKSPACE_DEFAULT, &want);
    cutensorPlan_t raw = nullptr;
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlan(h, &raw, tmp.op, tmp.pref, std::min<uint64_t>(want, budget));
    pl.contraction.reset(raw);
    if (st == CUTENSOR_STATUS_SUCCESS)
        st = cutensorPlanGetAttribute(h, raw, CUTENSOR_PLAN_REQUIRED_WORKSPACE, &pl.contractionWs, sizeof(uint64_t));
    return st;
}

// The contraction's workspace lies behind the regions handed out so far; `fixed` is their size.
static void finish_workspace(PlanContext& c, uint64_t fixed) {
    c.pl.contractionOff = (int64_t)fixed;
    c.pl.requiredDevice = fixed + (uint64_t)round_up((int64_t)c.pl.contractionWs, 256);
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------
// One transfer src -> q of the part of cell `cell` of operand k that q needs, on the side this rank is on.  Offsets are relative to the
// send / receive region until plan_transfers knows where the regions start.
static cutensorStatus_t add_transfer(PlanContext& c, int k, int q, int64_t cell, const Box& need, WorkspaceLayout& sendWs, WorkspaceLayout& recvWs) {
    GatherPlan& G = *c.pl.gather;
    const MpTensor& x = c.pl.desc.operand(k);
    const int me = c.pl.rank, src = x.owner[(size_t)cell];
    if (src == q || (src != me && q != me)) return CUTENSOR_STATUS_SUCCESS;
    const Box cb = cell_box(x, cell);
    const Box part = intersect(need, cb);
    if (part.empty()) return CUTENSOR_STATUS_SUCCESS;
    Transfer t;
    t.tensor = k; t.src = src; t.dst = q; t.box = part;
    t.bytes = part.volume() * (int64_t)elem_size(x.dtype);
    if (src == me) {
        t.direct = x.packed && part == cb && sizes(cb) == x.bs;
        if (!t.direct) {
            t.sendOff = sendWs.take(t.bytes).off;
            const cutensorStatus_t st = make_copy(c.handle->h, x.dtype, copy_modes(part, x.elemStride, packed_strides(sizes(part))), t.pack,
                                                  box_offset(part, cb, x.elemStride), 0);
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
        }
        G.sends.push_back(std::move(t));
    } else {
        t.inPlace = part == need;
        if (!t.inPlace) t.recvOff = recvWs.take(t.bytes).off;
        G.recvs.push_back(std::move(t));
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// Transfers (tensor, receiver q, cell) in a fixed order both sides agree on; where this rank is the receiver, whether the operand is
// used in place.  Takes the send and the receive region.
cutensorStatus_t plan_transfers(PlanContext& c) {
    GatherPlan& G = *c.pl.gather;
    const cutensorMpOperationDescriptor& d = c.pl.desc;
    const int me = c.pl.rank;
    WorkspaceLayout sendWs, recvWs;
    for (int k = 0; k < 2; ++k) {
        const MpTensor& x = d.operand(k);
        const Box myCell = block_of_rank(x, me);
        for (int q = 0; q < c.pl.nranks; ++q) {
            if (c.cBox[(size_t)q].empty()) continue;
            const Box need = needed_box(x, d.modes(k), d.mC, c.cBox[(size_t)q]);
            if (q == me) {
                OperandPlan& o = G.in[k];
                o.need = need;
                o.staged = !(intersect(need, myCell) == need);        // in place only when the rank's own block covers the whole box
                if (!o.staged) { o.viewOff = box_offset(need, myCell, x.elemStride); o.viewStride = x.elemStride; }
            }
            if (x.replicated()) continue;        // every rank already holds all of it
            for (int64_t cell = 0; cell < x.numCells; ++cell) {
                const cutensorStatus_t st = add_transfer(c, k, q, cell, need, sendWs, recvWs);
                if (st != CUTENSOR_STATUS_SUCCESS) return st;
            }
        }
    }
    G.send = c.ws.take(sendWs.end());
    G.recv = c.ws.take(recvWs.end());
    for (Transfer& t : G.sends) if (!t.direct) t.sendOff += G.send.off;
    for (Transfer& t : G.recvs) if (!t.inPlace) t.recvOff += G.recv.off;
    return CUTENSOR_STATUS_SUCCESS;
}

// Staging tensors of the operands not used in place, with the copies that fill them: the rank's own part, and every received part that
// did not arrive in place.
cutensorStatus_t plan_staging(PlanContext& c) {
    GatherPlan& G = *c.pl.gather;
    cutensorHandle_t h = c.handle->h;
    G.stage.off = c.ws.end();
    for (int k = 0; k < 2 && c.pl.compute; ++k) {
        const MpTensor& x = c.pl.desc.operand(k);
        OperandPlan& o = G.in[k];
        if (!o.staged) continue;
        const std::vector<int64_t> stStride = packed_strides(sizes(o.need));
        o.stage = c.ws.take(o.need.volume() * (int64_t)elem_size(x.dtype));
        o.viewStride = stStride;
        const Box myCell = block_of_rank(x, c.pl.rank);
        const Box own = intersect(o.need, myCell);
        if (!own.empty()) {
            CopyOp copy;
            const cutensorStatus_t st = make_copy(h, x.dtype, copy_modes(own, x.elemStride, stStride), copy, box_offset(own, myCell, x.elemStride),
                                                  box_offset(own, o.need, stStride));
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
            o.localCopies.push_back(std::move(copy));
        }
        for (Transfer& t : G.recvs) {
            if (t.tensor != k) continue;
            if (t.inPlace) { t.recvOff = o.stage.off; continue; }
            const cutensorStatus_t st = make_copy(h, x.dtype, copy_modes(t.box, packed_strides(sizes(t.box)), stStride), t.unpack, 0,
                                                  box_offset(t.box, o.need, stStride));
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
        }
    }
    G.stage.bytes = c.ws.end() - G.stage.off;
    return CUTENSOR_STATUS_SUCCESS;
}

// Staged (or in-place) views of A and B, D written straight into the rank's own block.
cutensorStatus_t plan_gather_contraction(PlanContext& c) {
    const GatherPlan& G = *c.pl.gather;
    const cutensorMpOperationDescriptor& d = c.pl.desc;
    const uint64_t fixed = (uint64_t)c.ws.end();
    if (fixed > c.devLimit) return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
    if (c.pl.compute) {
        TensorView view[3];
        for (int k = 0; k < 2; ++k) {
            const OperandPlan& o = G.in[k];
            view[k] = TensorView{sizes(o.need), o.viewStride, o.staged ? 256u : alignment_of(o.viewOff * (int64_t)elem_size(d.A.dtype))};
        }
        view[2] = TensorView{sizes(c.cBox[(size_t)c.pl.rank]), d.C.elemStride, 256u};
        const cutensorStatus_t st = plan_local_contraction(c, view, c.devLimit - fixed);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
    }
    finish_workspace(c, fixed);
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------
// Replicated C: the partial lives in the user's D when that is the packed whole C, else in a staged copy; one all-reduce.
cutensorStatus_t plan_reduce_replicated(PlanContext& c) {
    ReducePlan& R = *c.pl.reduce;
    const MpTensor& C = c.pl.desc.C;
    cutensorHandle_t h = c.handle->h;
    const int64_t es = (int64_t)elem_size(C.dtype);
    const std::vector<int64_t> pStride = packed_strides(C.extent);
    const Box whole = whole_box(C.extent);
    R.direct = C.packed && C.bs == C.extent;
    if (!R.direct) {
        R.stage = c.ws.take(R.cElems * es);
        cutensorStatus_t st = make_copy(h, C.dtype, copy_modes(whole, C.elemStride, pStride), R.cIn);
        if (st == CUTENSOR_STATUS_SUCCESS) st = make_copy(h, C.dtype, copy_modes(whole, pStride, C.elemStride), R.out);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
    }
    if (c.handle->transport->needs_scratch()) R.scratch = c.ws.take(R.cElems * es);
    return CUTENSOR_STATUS_SUCCESS;
}

// the destination blocks are already equal contiguous slots of the packed partial, in rank order
static bool blocks_are_slots(const std::vector<Box>& cBox, const std::vector<int64_t>& full, int64_t slotElems) {
    const std::vector<int64_t> pStride = packed_strides(full);
    const Box whole = whole_box(full);
    for (size_t q = 0; q < cBox.size(); ++q) {
        const Box& b = cBox[q];
        if (b.empty() || b.volume() != slotElems || !contiguous_in(b, full) || box_offset(b, whole, pStride) != (int64_t)q * slotElems) return false;
    }
    return true;
}

// Distributed C: a staged full-size partial, the destination blocks packed into equal slots of a send region unless they already are
// such slots, one reduce-scatter, the received slot unpacked into the rank's block of D unless that block is the slot.
cutensorStatus_t plan_reduce_scattered(PlanContext& c) {
    ReducePlan& R = *c.pl.reduce;
    const MpTensor& C = c.pl.desc.C;
    cutensorHandle_t h = c.handle->h;
    const int world = c.pl.nranks;
    const int64_t es = (int64_t)elem_size(C.dtype);
    const std::vector<int64_t> pStride = packed_strides(C.extent);
    const Box whole = whole_box(C.extent);
    const Box& myC = c.cBox[(size_t)c.pl.rank];
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    R.stage = c.ws.take(R.cElems * es);
    if (!myC.empty()) {
        st = make_copy(h, C.dtype, copy_modes(myC, C.elemStride, pStride), R.cIn, 0, box_offset(myC, whole, pStride));
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
    }
    for (const Box& b : c.cBox) R.slotElems = std::max(R.slotElems, b.volume());
    R.slotElems = std::max<int64_t>(R.slotElems, 1);
    R.packDirect = blocks_are_slots(c.cBox, C.extent, R.slotElems);
    if (!R.packDirect) {
        R.send = c.ws.take((int64_t)world * R.slotElems * es);
        R.pack.resize((size_t)world);
        for (int q = 0; q < world; ++q) {
            const Box& b = c.cBox[(size_t)q];
            if (b.empty()) continue;
            st = make_copy(h, C.dtype, copy_modes(b, pStride, packed_strides(sizes(b))), R.pack[(size_t)q], box_offset(b, whole, pStride),
                           (int64_t)q * R.slotElems);
            if (st != CUTENSOR_STATUS_SUCCESS) return st;
        }
    }
    R.recvDirect = !myC.empty() && C.packed && sizes(myC) == C.bs && myC.volume() == R.slotElems;
    if (!R.recvDirect) {
        R.recv = c.ws.take(R.slotElems * es);
        if (!myC.empty()) st = make_copy(h, C.dtype, copy_modes(myC, packed_strides(sizes(myC)), C.elemStride), R.unpack);
    }
    return st;
}

// Own blocks of A and B in place, the partial (or the user's D) as packed full-size C.
cutensorStatus_t plan_reduce_contraction(PlanContext& c) {
    const cutensorMpOperationDescriptor& d = c.pl.desc;
    const uint64_t fixed = (uint64_t)c.ws.end();
    if (fixed > c.devLimit) return CUTENSOR_STATUS_INSUFFICIENT_WORKSPACE;
    const TensorView view[3] = {TensorView{sizes(block_of_rank(d.A, c.pl.rank)), d.A.elemStride, 256u},
                                TensorView{sizes(block_of_rank(d.B, c.pl.rank)), d.B.elemStride, 256u},
                                TensorView{d.C.extent, packed_strides(d.C.extent), 256u}};
    const cutensorStatus_t st = plan_local_contraction(c, view, c.devLimit - fixed);
    if (st != CUTENSOR_STATUS_SUCCESS) return st;
    c.pl.compute = true;     // every rank contracts its K slice, whether or not it owns a block of C
    finish_workspace(c, fixed);
    return CUTENSOR_STATUS_SUCCESS;
}

}  // namespace ctamd_mp
