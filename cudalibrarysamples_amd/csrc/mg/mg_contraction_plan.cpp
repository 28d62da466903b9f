// mg_contraction_plan.cpp — the steps of cutensorMgCreateContractionPlan (mg.cpp runs them in this order; the algorithm is described at
// the top of that file).  Each step is a function of the handle / descriptor (PlanInputs) and the results of earlier steps.  The order of
// every loop here fixes the order of pieces, transfers, waves and events of a plan (tests/golden/mg_plan_descriptions.json.gz).
#include <algorithm>
#include <map>
#include <set>
#include <tuple>

#include "mg_internal.hpp"

namespace ctamd_mg {

// Upper bound of the staging images (whether a tensor needs staging at all is decided by the plan; the workspace
// query must not be smaller than what any plan of this descriptor can ask for).
void staging_sizes(const cutensorMgContractionDescriptor& d, int64_t out[3]) {
    const size_t es = elem_size(d.A.dtype);
    auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
    out[0] = up(d.A.numCells * d.A.cellElems * (int64_t)es);
    out[1] = up(d.B.numCells * d.B.cellElems * (int64_t)es);
    out[2] = up(d.C.numCells * d.C.cellElems * (int64_t)es);
}

int waves_wanted() {
    const char* e = std::getenv("CUTENSORMG_AMD_WAVES");
    return e != nullptr ? std::max(1, std::atoi(e)) : 1;
}

void PlanDeleter::operator()(cutensorMgContractionPlan* plan) const {
    if (plan == nullptr) return;
    for (Piece& p : plan->pieces) {
        for (auto& sub : p.subs) cutensorDestroyPlan(sub.plan);
        for (auto& s : p.scatter) cutensorDestroyPlan(s.plan);
    }
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
            for (int e = plan->ev.start(g); e < plan->ev.start(g + 1); ++e)
                if (plan->events[(size_t)e]) (void)hipEventDestroy(plan->events[(size_t)e]);
        }
    }
    delete plan;
}

// ---- label universe, block-index digits per label ----------------------------------------------
cutensorStatus_t build_radix(const PlanInputs& in, Labels* lab) {
    const Operands& o = in.ops;
    for (int k = 0; k < 3; ++k)
        for (int32_t l : *o.M[k])
            if (find_label(lab->universe, l) < 0) lab->universe.push_back(l);
    lab->radix.assign(lab->universe.size(), Radix());
    for (size_t li = 0; li < lab->universe.size(); ++li) {
        std::set<int64_t> dcs;
        Radix& r = lab->radix[li];
        for (int k = 0; k < 3; ++k) {
            const int i = find_label(*o.M[k], lab->universe[li]);
            if (i < 0) continue;
            r.blockSize = o.T[k]->blockSize[i];
            r.numBlocks = o.T[k]->localBlocks[i] * o.T[k]->deviceCount[i];      // padded: whole blocks per cell
            dcs.insert(o.T[k]->deviceCount[i]);
        }
        int64_t prev = 1;
        for (int64_t dc : dcs) {          // ascending; each divides the next (checked by the contraction descriptor)
            if (dc % prev != 0) return CUTENSOR_STATUS_NOT_SUPPORTED;
            if (dc / prev > 1) r.f.push_back(dc / prev);
            prev = dc;
        }
        if (r.numBlocks / prev > 1) r.f.push_back(r.numBlocks / prev);
        if ((int)r.f.size() > kMaxDigits) return CUTENSOR_STATUS_NOT_SUPPORTED;
    }
    return CUTENSOR_STATUS_SUCCESS;
}

namespace {

// index in C of the largest mode that is free (in exactly one of A / B) — else any C mode
int pick_p(const cutensorMgContractionDescriptor& d) {
    int pC = -1;
    for (int pass = 0; pass < 2 && pC < 0; ++pass)
        for (uint32_t i = 0; i < d.C.n; ++i) {
            const bool inA = find_label(d.mA, d.mC[i]) >= 0, inB = find_label(d.mB, d.mC[i]) >= 0;
            if (pass == 0 && inA == inB) continue;
            if (pC < 0 || d.C.extent[i] > d.C.extent[pC]) pC = (int)i;
        }
    return pC;
}

// Y = the operand that does not carry p (gathered whole); q = Y's free mode with the largest device count whose
// grid coordinate is ONE digit in Y (so that a run of coordinates is a box)
void pick_q(const PlanInputs& in, const Labels& lab, Sharding* sh) {
    const cutensorMgContractionDescriptor& d = in.d;
    if (sh->pC >= 0) sh->yK = find_label(d.mA, d.mC[sh->pC]) >= 0 ? 1 : 0;
    if (sh->pC >= 0 && find_label(d.mA, d.mC[sh->pC]) >= 0 && find_label(d.mB, d.mC[sh->pC]) >= 0) sh->yK = -1;   // batch mode: both carry it
    if (sh->yK < 0 || CTAMD_HOOK_IS("CUTENSORMG_AMD_QSPLIT", "0")) return;
    const MgTensor& Y = *in.ops.T[sh->yK];
    for (uint32_t i = 0; i < Y.n; ++i) {
        const int32_t l = (*in.ops.M[sh->yK])[i];
        if (find_label(d.mC, l) < 0 || Y.deviceCount[i] <= 1) continue;
        const int li = find_label(lab.universe, l);
        if (grid_digits(lab.radix[li], Y.deviceCount[i]) != 1) continue;
        if (Y.deviceCount[i] > sh->qCount) { sh->qCount = Y.deviceCount[i]; sh->qLi = li; sh->qDigit = 0; }
    }
}

// c shards of ceil(E / c) rounded up to 16 indices: are all of them non-empty?
bool all_busy(int64_t E, int c) {
    const int64_t per = ((E + c - 1) / c + 15) / 16 * 16;
    return per * (int64_t)(c - 1) < E;
}

// p is too short for one 16-aligned shard per device: cut it nP ways only (the largest divisor of the device count whose shards are
// all non-empty) and pick p2, a free mode with at least n2 = nDev / nP indices whose n2 shards cross the FEWEST block boundaries (every
// crossing is another piece, i.e. another local contraction), the longer one on a tie.  Returns nP; sh->p2C stays -1 when there is
// nothing else to cut (the old rule then: nP = nDev, some devices stay idle).
int pick_p2(const PlanInputs& in, Sharding* sh) {
    const cutensorMgContractionDescriptor& d = in.d;
    const int pC = sh->pC, nDev = in.nDev;
    int nP = 1;
    for (int c = 1; c <= nDev; ++c)
        if (nDev % c == 0 && all_busy(d.C.extent[pC], c)) nP = c;
    const bool pInA = find_label(d.mA, d.mC[pC]) >= 0;
    const int n2w = nDev / nP;
    auto segments = [&](uint32_t i) {
        const int64_t e = d.C.extent[i], b = d.C.blockSize[i], per2 = (e + n2w - 1) / n2w;
        int64_t segs = 0;
        for (int g2 = 0; g2 < n2w; ++g2) {
            const int64_t lo = (int64_t)g2 * per2, hi = std::min<int64_t>(e, lo + per2);
            if (lo < hi) segs += (hi - 1) / b - lo / b + 1;
        }
        return segs;
    };
    int p2C = -1;
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
    sh->p2C = p2C;
    return p2C < 0 ? nDev : nP;
}

// one shard of p (and of p2) per device, cut at block boundaries: device g works on (p shard g % nP, p2 shard g / nP)
void cut_shards(const PlanInputs& in, int nP, Sharding* sh) {
    const cutensorMgContractionDescriptor& d = in.d;
    const int pC = sh->pC, p2C = sh->p2C;
    const int64_t E = d.C.extent[pC], bs = d.C.blockSize[pC];
    const int n2 = (p2C >= 0) ? in.nDev / nP : 1;
    int64_t per = (E + nP - 1) / nP;
    per = (per + 15) / 16 * 16;   // keep shard starts 64-byte aligned for the vector kernels
    const int64_t E2 = p2C >= 0 ? d.C.extent[p2C] : 0, bs2 = p2C >= 0 ? d.C.blockSize[p2C] : 1;
    const int64_t per2 = p2C >= 0 ? (E2 + n2 - 1) / n2 : 0;
    for (int g = 0; g < in.nDev; ++g) {
        const int gp = g % nP, g2 = g / nP;
        int64_t lo = (int64_t)gp * per, hi = std::min<int64_t>(E, lo + per);
        while (lo < hi) {
            const int64_t cut = std::min<int64_t>(hi, (lo / bs + 1) * bs);
            if (p2C < 0) sh->shards.push_back(Shard{g, lo, cut, 0, 0});
            else {
                int64_t lo2 = (int64_t)g2 * per2, hi2 = std::min<int64_t>(E2, lo2 + per2);
                while (lo2 < hi2) {
                    const int64_t cut2 = std::min<int64_t>(hi2, (lo2 / bs2 + 1) * bs2);
                    sh->shards.push_back(Shard{g, lo, cut, lo2, cut2});
                    lo2 = cut2;
                }
            }
            lo = cut;
        }
    }
}

Shard shard_of(const Piece& p) { return Shard{p.dev, p.lo, p.hi, p.lo2, p.hi2}; }

// the restriction of the views to a shard and a run [c0, c1) of q's grid coordinate
Restrict restrict_of(const Sharding& sh, const Shard& s, int64_t c0, int64_t c1) {
    Restrict rs;
    if (sh.pC >= 0) { rs.pLabel = sh.pLi; rs.lo = s.lo; rs.hi = s.hi; }
    if (sh.p2Li >= 0 && s.hi2 > s.lo2) { rs.p2Label = sh.p2Li; rs.lo2 = s.lo2; rs.hi2 = s.hi2; }
    if (sh.qLi >= 0 && c1 > c0) { rs.qLabel = sh.qLi; rs.qDigit = sh.qDigit; rs.c0 = c0; rs.c1 = c1; }
    return rs;
}
Restrict restrict_of(const Sharding& sh, const Piece& p) { return restrict_of(sh, shard_of(p), p.q0, p.q1); }

}  // namespace

// ---- the mode to shard (p), the mode that orders the gather (q), and the shards ------------------------------------------------------
// Shards of p start at multiples of 16 indices (64-byte aligned rows for the vector kernels).  When p is too short for one such
// shard per device (blog_post.cu on 8 devices: its largest free mode has 16 .. 96 indices at scaling 1 .. 12, :155-175) that rule
// alone leaves devices without work: p is then cut nP ways only and a SECOND free mode p2 of C — the largest other one, preferably
// carried by the other operand so that both operands shrink per device — is cut n2 = devices / nP ways (plain ceil() shards: these
// modes are small, alignment is not the concern).  The gather-ordering mode q is not used together with p2.
Sharding choose_sharding(const PlanInputs& in, const Labels& lab) {
    const cutensorMgContractionDescriptor& d = in.d;
    Sharding sh;
    sh.pC = pick_p(d);
    sh.pLi = sh.pC >= 0 ? find_label(lab.universe, d.mC[sh.pC]) : -1;
    pick_q(in, lab, &sh);
    if (sh.pC < 0) {
        sh.shards.push_back(Shard{0, 0, 0, 0, 0});
        return sh;
    }
    int nP = in.nDev;
    if (!all_busy(d.C.extent[sh.pC], in.nDev) && !CTAMD_HOOK_IS("CUTENSORMG_AMD_SHARD2", "0")) nP = pick_p2(in, &sh);
    if (sh.p2C >= 0) { sh.p2Li = find_label(lab.universe, d.mC[sh.p2C]); sh.qLi = -1; sh.qDigit = -1; sh.qCount = 1; }
    cut_shards(in, nP, &sh);
    return sh;
}

// ---- pieces: the shards of a device, then runs of q's coordinate; alternating compute streams -----------------------------------------
std::vector<Piece> cut_pieces(const PlanInputs& in, const Labels& lab, const Sharding& sh) {
    const Operands& o = in.ops;
    // is every cell of Y that the restricted view touches local to device g?
    auto all_local = [&](const Restrict& rs, int g) {
        for (int c : cells_of(*o.T[sh.yK], *o.M[sh.yK], lab.universe, lab.radix, rs))
            if (o.T[sh.yK]->devices[c] != in.h->devices[g]) return false;
        return true;
    };
    const int64_t qCount = sh.qCount;
    std::vector<Piece> pieces;
    for (int g = 0; g < in.nDev; ++g) {
        std::vector<Piece> mine;
        for (const Shard& s : sh.shards) {
            if (s.dev != g) continue;
            if (sh.qLi < 0) {
                Piece p; p.dev = g; p.lo = s.lo; p.hi = s.hi; p.lo2 = s.lo2; p.hi2 = s.hi2;
                mine.push_back(p);
                continue;
            }
            // class of each q coordinate: -1 = everything this coordinate needs of Y is already on the device, else the
            // gather wave that brings it (ring distance from the device's own position, wavesWanted waves)
            std::vector<int> cls((size_t)qCount);
            for (int64_t c = 0; c < qCount; ++c) {
                if (all_local(restrict_of(sh, s, c, c + 1), g)) { cls[(size_t)c] = -1; continue; }
                const int64_t dist = ((c - g) % qCount + qCount) % qCount;      // 1 .. qCount - 1 for the usual one-cell-per-device layout
                cls[(size_t)c] = (int)std::min<int64_t>(in.wavesWanted - 1, (dist > 0 ? dist - 1 : 0) * in.wavesWanted / std::max<int64_t>(1, qCount - 1));
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
    return pieces;
}

namespace {

// (device, tensor, cell) -> index of the transfer that brings the cell into the device's staging image
class TransferIndex {
public:
    int find(int dev, int tensor, int cell) const {
        const auto it = map_.find(std::make_tuple(dev, tensor, cell));
        return it == map_.end() ? -1 : it->second;
    }
    void add(int dev, int tensor, int cell, int index) { map_[std::make_tuple(dev, tensor, cell)] = index; }
private:
    std::map<std::tuple<int, int, int>, int> map_;
};

// operand uses of every piece, and one transfer per (device, staged cell) in first-use order; returns which tensors are staged at all
void plan_operand_uses(const PlanInputs& in, const Labels& lab, const Sharding& sh, cutensorMgContractionPlan* pl, TransferIndex* have, bool staged[3]) {
    const Operands& o = in.ops;
    double flopsAll = 2.0;
    for (size_t li = 0; li < lab.universe.size(); ++li) flopsAll *= (double)(lab.radix[li].blockSize * lab.radix[li].numBlocks);
    for (Piece& p : pl->pieces) {
        const Restrict rs = restrict_of(sh, p);
        p.flops = flopsAll;
        if (sh.pC >= 0) p.flops *= (double)(p.hi - p.lo) / (double)in.d.C.extent[sh.pC];
        if (sh.p2C >= 0 && p.hi2 > p.lo2) p.flops *= (double)(p.hi2 - p.lo2) / (double)in.d.C.extent[sh.p2C];
        if (sh.qLi >= 0) p.flops *= (double)(p.q1 - p.q0) / (double)sh.qCount;
        for (int k = 0; k < 3; ++k) {
            OperandUse& u = p.use[k];
            u.cells = cells_of(*o.T[k], *o.M[k], lab.universe, lab.radix, rs);
            u.direct = u.cells.size() == 1 && o.T[k]->devices[u.cells[0]] == in.h->devices[p.dev] &&
                       !CTAMD_HOOK_IS("CUTENSORMG_AMD_DIRECT", "0") && !(in.h->forceGather && k < 2);
            if (u.direct) { u.cell = u.cells[0]; continue; }
            staged[k] = true;
            for (int c : u.cells) {
                if (have->find(p.dev, k, c) >= 0) continue;
                Transfer t;
                t.tensor = k; t.cell = c; t.dst = p.dev;
                t.ownerDevice = o.T[k]->devices[c];
                t.src = device_rank(in.h, t.ownerDevice);
                // forced gather: an own cell of an operand is NOT a device copy on the caller's stream — it goes the remote way (RCCL
                // to itself / a peer copy onto the same device) on the communication stream, with its wave event
                t.local = t.ownerDevice == in.h->devices[p.dev] && !(in.h->forceGather && k < 2);
                t.bytes = o.T[k]->cellElems * (int64_t)in.es;
                have->add(p.dev, k, c, (int)pl->transfers.size());
                pl->transfers.push_back(t);
            }
        }
    }
}

// waves of the remote transfers: in the order the pieces of the receiving device first need them; returns the number of waves
int assign_waves(const PlanInputs& in, const TransferIndex& have, cutensorMgContractionPlan* pl) {
    std::vector<std::vector<int>> order((size_t)in.nDev);   // remote transfer indices per device in first-use order
    std::set<int> seen;
    for (const Piece& p : pl->pieces)
        for (int k = 0; k < 3; ++k) {
            if (p.use[k].direct) continue;
            for (int c : p.use[k].cells) {
                const int ti = have.find(p.dev, k, c);
                if (pl->transfers[(size_t)ti].local || seen.count(ti)) continue;
                seen.insert(ti);
                order[(size_t)p.dev].push_back(ti);
            }
        }
    int numWaves = 0;
    for (int g = 0; g < in.nDev; ++g) {
        const size_t n = order[(size_t)g].size();
        const size_t perWave = std::max<size_t>(1, (n + (size_t)in.wavesWanted - 1) / (size_t)in.wavesWanted);
        for (size_t i = 0; i < n; ++i) {
            Transfer& t = pl->transfers[(size_t)order[(size_t)g][i]];
            t.wave = (int)(i / perWave);
            numWaves = std::max(numWaves, t.wave + 1);
        }
    }
    return numWaves;
}

// RCCL: one event per (device, wave); peer copies: one event per (device, wave, comm stream), a wave's copies spread over the streams
void assign_events(cutensorMgContractionPlan* pl, int nDev) {
    std::map<std::pair<int, int>, int> n;   // (device, wave) -> remote transfers so far
    for (Transfer& t : pl->transfers) {
        if (t.local) continue;
        int& k = n[std::make_pair(t.dst, t.wave)];
        t.event = pl->ev.wave(t.dst, t.wave, k % pl->ev.slotsPerWave);
        ++k;
    }
    pl->liveAtBetaZero.assign((size_t)pl->ev.start(nDev), 0);
    for (const Transfer& t : pl->transfers)
        if (!t.local && t.tensor != 2) pl->liveAtBetaZero[(size_t)t.event] = 1;
}

}  // namespace

// ---- operand uses, transfers, waves, events, the events every piece waits for, which staging images exist ----------------------------
void plan_transfers(const PlanInputs& in, const Labels& lab, const Sharding& sh, cutensorMgContractionPlan* pl) {
    TransferIndex have;
    bool staged[3] = {false, false, false};
    plan_operand_uses(in, lab, sh, pl, &have, staged);
    const int numWaves = assign_waves(in, have, pl);
    pl->ev = EventLayout(pl->useRccl ? 1 : std::max(1, std::min(7, in.nDev - 1)), numWaves, pl->useRccl);
    assign_events(pl, in.nDev);
    for (Piece& p : pl->pieces) {
        std::set<int> ev;
        for (int k = 0; k < 3; ++k) {
            if (p.use[k].direct) continue;
            for (int c : p.use[k].cells) {
                const Transfer& t = pl->transfers[(size_t)have.find(p.dev, k, c)];
                if (!t.local) ev.insert(t.event);
            }
        }
        p.waitEvents.assign(ev.begin(), ev.end());
    }
    for (int k = 0; k < 3; ++k)
        if (!staged[k]) pl->stagingBytes[k] = 0;
}

// ---- all-gather eligibility, the transport switch, whose streams a device's reads hold up, which helper streams a device uses --------
void classify_transport(const PlanInputs& in, cutensorMgContractionPlan* pl) {
    const cutensorMgHandle* handle = in.h;
    const int nDev = in.nDev;
    // all-gather eligibility per tensor (a property of the layout; whether RCCL is there is a property of the handle)
    for (int k = 0; k < 2; ++k) {   // operands only: C is gathered only for beta != 0 and scattered back, never all-gathered
        const MgTensor& t = *in.ops.T[k];
        bool ok = handle->distinct && (nDev > 1 || handle->forceGather) && t.numCells == nDev;
        for (int c = 0; ok && c < nDev; ++c) ok = t.devices[(size_t)c] == handle->devices[(size_t)c];
        std::vector<int> remote((size_t)nDev, 0);
        for (const Transfer& tr : pl->transfers)
            if (tr.tensor == k && !tr.local) { ++remote[(size_t)tr.dst]; ok = ok && tr.wave == 0; }
        // every device receives every cell it does not hold (forced gather: its own one too — the collective delivers all nDev anyway)
        for (int g = 0; ok && g < nDev; ++g) ok = remote[(size_t)g] == (handle->forceGather ? nDev : nDev - 1);
        pl->allGatherEligible[k] = ok;
    }
    pl->transport = env_is("CUTENSORMG_AMD_TRANSPORT", "allgather") ? 1 : env_is("CUTENSORMG_AMD_TRANSPORT", "sendrecv") ? 2 : 0;
    pl->readOwners.assign((size_t)nDev, {});
    for (const Transfer& t : pl->transfers) {
        if (t.local) continue;
        std::vector<int>& v = pl->readOwners[(size_t)t.dst];
        for (int o = 0; o < nDev; ++o)
            if (o != t.dst && handle->devices[(size_t)o] == t.ownerDevice && std::find(v.begin(), v.end(), o) == v.end()) v.push_back(o);
    }
    pl->usesAux.assign((size_t)nDev, 0);
    pl->usesComm.assign((size_t)nDev, 0);
    for (const Piece& p : pl->pieces) if (p.stream != 0) pl->usesAux[(size_t)p.dev] = 1;
    for (const Transfer& t : pl->transfers)
        if (!t.local) { pl->usesComm[(size_t)t.dst] = 1; if (t.src >= 0) pl->usesComm[(size_t)t.src] = 1; }
}

// ---- boxes of the contracted index space (one, unless a contracted mode is ragged): the cartesian product of kbox_list() -------------
cutensorStatus_t contracted_boxes(const PlanInputs& in, const Labels& lab, Boxes* boxes) {
    boxes->assign(1, {});
    for (size_t li = 0; li < lab.universe.size(); ++li) {
        if (find_label(in.d.mC, lab.universe[li]) >= 0) continue;              // a mode of C: padded, never clipped
        int64_t extent = 0;
        for (int k = 0; k < 2; ++k) {
            const int i = find_label(*in.ops.M[k], lab.universe[li]);
            if (i >= 0) extent = in.ops.T[k]->extent[(size_t)i];
        }
        if (extent == lab.radix[li].blockSize * lab.radix[li].numBlocks) continue;   // fills the padded space
        const std::vector<Clip> mine = kbox_list((int)li, lab.radix[li], extent);
        Boxes next;
        for (const auto& b : *boxes)
            for (const Clip& c : mine) { next.push_back(b); next.back().push_back(c); }
        boxes->swap(next);
    }
    if (boxes->empty() || boxes->size() > 64) return CUTENSOR_STATUS_NOT_SUPPORTED;
    // 16-bit data: boxes accumulate through D, which would round every partial sum to the 16-bit type (the kernels' contract is fp32
    // accumulation and one rounding) — a ragged contracted mode stays unsupported for these types
    if (boxes->size() > 1 && in.es == 2) return CUTENSOR_STATUS_NOT_SUPPORTED;
    return CUTENSOR_STATUS_SUCCESS;
}

namespace {

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

// the single-GPU library's descriptors a local plan is built from: released when the plan exists (or could not be made)
struct LocalHandles {
    cutensorTensorDescriptor_t t[3] = {nullptr, nullptr, nullptr};
    cutensorOperationDescriptor_t op = nullptr;
    cutensorPlanPreference_t pref = nullptr;
    LocalHandles() = default;
    LocalHandles(const LocalHandles&) = delete;
    LocalHandles& operator=(const LocalHandles&) = delete;
    ~LocalHandles() {
        cutensorDestroyOperationDescriptor(op);
        cutensorDestroyPlanPreference(pref);
        for (int k = 0; k < 3; ++k) cutensorDestroyTensorDescriptor(t[k]);
    }
};

void host_view(const View& v, Piece::HostView* hv) { hv->extent = v.extent; hv->stride = v.stride; hv->modes = v.modes; }

// one local contraction plan on the views of the piece under the restriction rs (clips included)
cutensorStatus_t make_sub(const PlanInputs& in, const Labels& lab, const Restrict& rs, const Piece& p, uint64_t wsLimit, Piece::Sub* sub) {
    cutensorHandle_t h = in.h->handles[p.dev];
    View v[3];
    for (int k = 0; k < 3; ++k) {
        v[k] = make_view(*in.ops.T[k], *in.ops.M[k], lab.universe, lab.radix, rs, !p.use[k].direct);
        sub->off[k] = v[k].offset;
        host_view(v[k], &sub->hv[k]);
    }
    LocalHandles l;
    cutensorStatus_t st = CUTENSOR_STATUS_SUCCESS;
    for (int k = 0; k < 3 && st == CUTENSOR_STATUS_SUCCESS; ++k) st = make_desc(h, v[k], in.ops.T[k]->dtype, &l.t[k]);
    if (st == CUTENSOR_STATUS_SUCCESS)
        st = cutensorCreateContraction(h, &l.op, l.t[0], v[0].modes.data(), CUTENSOR_OP_IDENTITY, l.t[1], v[1].modes.data(), CUTENSOR_OP_IDENTITY,
                                       l.t[2], v[2].modes.data(), CUTENSOR_OP_IDENTITY, l.t[2], v[2].modes.data(), compute_desc(in.d.compute));
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlanPreference(h, &l.pref, CUTENSOR_ALGO_DEFAULT, CUTENSOR_JIT_MODE_NONE);
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlan(h, &sub->plan, l.op, l.pref, wsLimit);
    if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorPlanGetAttribute(h, sub->plan, CUTENSOR_PLAN_REQUIRED_WORKSPACE, &sub->ws, sizeof(sub->ws));
    if (st != CUTENSOR_STATUS_SUCCESS) { cutensorDestroyPlan(sub->plan); sub->plan = nullptr; }
    return st;
}

// Which block-index digit of a local plan's mode table to peel: a digit (not w) of a group with more than four unfusable modes, with
// the smallest extent; never a digit of the contracted group for 16-bit data (it would accumulate through D).  -1: none.
int pick_peel_digit(int nm, const int32_t* grp, const int32_t* lab, const int64_t* ext, size_t es) {
    int count[4] = {0, 0, 0, 0};
    for (int i = 0; i < nm; ++i) ++count[grp[i]];
    int best = -1;
    for (int i = 0; i < nm; ++i) {
        if (count[grp[i]] <= 4 || (lab[i] & 7) == 7 || ext[i] < 2) continue;        // only digits (not w) of an oversized group
        if (es == 2 && grp[i] == 3) continue;                                     // 16-bit data: never accumulate through D
        if (best < 0 || ext[i] < ext[best]) best = i;
    }
    return best;
}

// a work item of build_local_plans: a clip set and whether an earlier item already writes its region of D
struct Work { std::vector<Clip> clips; bool acc; };

// Peels digit `digit` of label li out of the clip set `box`: one work item per value, pushed in reverse (executed in ascending order).
// false: the digit is not peelable (a sharded mode, or a single value left).
bool peel(const PlanInputs& in, const Labels& lab, const Restrict& rs, const std::vector<Clip>& box, bool boxAcc, int li, int digit, std::vector<Work>* todo) {
    std::vector<Clip> base = box;
    Clip* c = nullptr;
    for (Clip& x : base) if (x.label == li) c = &x;
    if (c == nullptr) {        // first restriction of this label: everything it had in the view
        Clip fresh;
        fresh.label = li;
        fresh.wHi = lab.radix[(size_t)li].blockSize;
        for (size_t j = 0; j < lab.radix[(size_t)li].f.size(); ++j) fresh.digit.push_back({0, lab.radix[(size_t)li].f[j]});
        if (li == rs.qLabel && rs.qDigit >= 0) fresh.digit[(size_t)rs.qDigit] = {rs.c0, rs.c1};   // the piece's run of q's coordinate
        base.push_back(fresh);
        c = &base.back();
    }
    const std::pair<int64_t, int64_t> range = c->digit[(size_t)digit];
    if (rs.is_p(li) || range.second - range.first < 2) return false;
    const bool contractedDigit = find_label(in.d.mC, lab.universe[(size_t)li]) < 0;
    for (int64_t val = range.second - 1; val >= range.first; --val) {
        c->digit[(size_t)digit] = {val, val + 1};
        todo->push_back(Work{base, boxAcc || (contractedDigit && val > range.first)});
    }
    return true;
}

}  // namespace

// ---- the local contractions of a piece ------------------------------------------------------------------------------------------------
// Work list of clip sets: the boxes of the contracted index space, each possibly split further ("peeled").  acc: an earlier entry
// already writes this region of D — every box after the first (the boxes tile the CONTRACTED index space, all cover the piece's whole
// output), and every value but the first of a peeled contracted digit; peeled free digits inherit.
// Peeling: a local view with more than four unfusable modes in a group (block-cyclic (w, digit, digit...) splits of several modes —
// blog_post.cu on 8 devices, scaling >= 2) would run on the functional mode-table kernel (measured 650 GFLOP/s against 70,000+ for the
// tiled kernels).  Instead one block-index digit of the oversized group — the one with the smallest extent — is taken out of the view
// and walked by the host: extent-many tiled contractions.
cutensorStatus_t build_local_plans(const PlanInputs& in, const Labels& lab, const Sharding& sh, const Boxes& boxes, Piece& p, cutensorMgContractionPlan* pl) {
    if (in.h->haveDevice) { (void)hipSetDevice(in.h->devices[p.dev]); (void)hipGetLastError(); }
    Restrict rs = restrict_of(sh, p);
    std::vector<Work> todo;
    for (size_t bi = boxes.size(); bi-- > 0;) todo.push_back(Work{boxes[bi], bi > 0});
    while (!todo.empty()) {
        const std::vector<Clip> box = todo.back().clips;
        const bool boxAcc = todo.back().acc;
        todo.pop_back();
        rs.clips = box;
        Piece::Sub sub;
        const cutensorStatus_t st = make_sub(in, lab, rs, p, pl->contractionWs, &sub);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        if (p.subs.empty()) for (int k = 0; k < 3; ++k) p.use[k].off = sub.off[k];
        int32_t grp[64], mlab[64];
        int64_t ext[64];
        const int nm = (p.subs.size() + todo.size() < 512) ? ctamdPlanModeTableGroups(sub.plan, grp, mlab, ext, 64) : 0;
        const int best = (nm > 0 && !CTAMD_HOOK_IS("CUTENSORMG_AMD_PEEL", "0")) ? pick_peel_digit(std::min(nm, 64), grp, mlab, ext, in.es) : -1;
        if (best >= 0 && peel(in, lab, rs, box, boxAcc, mlab[best] >> 3, mlab[best] & 7, &todo)) {
            cutensorDestroyPlan(sub.plan);
            ++pl->peeled;
            continue;
        }
        sub.accumulate = boxAcc;
        p.subs.push_back(sub);
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- scatter plans: the piece's region inside every cell of C it touches (cell-relative strides) -------------------------------------
cutensorStatus_t build_scatter_plans(const PlanInputs& in, const Labels& lab, const Sharding& sh, Piece& p) {
    if (p.use[2].direct) return CUTENSOR_STATUS_SUCCESS;
    cutensorHandle_t h = in.h->handles[p.dev];
    const View cellView = make_view(in.d.C, in.d.mC, lab.universe, lab.radix, restrict_of(sh, p), false);
    for (int c : p.use[2].cells) {
        LocalHandles l;
        Piece::Scatter sc{c, cellView.offset, nullptr, {}};
        host_view(cellView, &sc.hv);
        cutensorStatus_t st = make_desc(h, cellView, in.d.C.dtype, &l.t[0]);
        if (st == CUTENSOR_STATUS_SUCCESS)
            st = cutensorCreatePermutation(h, &l.op, l.t[0], cellView.modes.data(), CUTENSOR_OP_IDENTITY, l.t[0], cellView.modes.data(), compute_desc(in.d.compute));
        if (st == CUTENSOR_STATUS_SUCCESS) st = cutensorCreatePlan(h, &sc.plan, l.op, nullptr, 0);
        if (st != CUTENSOR_STATUS_SUCCESS) return st;
        p.scatter.push_back(sc);
    }
    return CUTENSOR_STATUS_SUCCESS;
}

// ---- who stores into whose cells of D from afar (the owners' caller streams must end behind those stores) -----------------------------
void scatter_owners(const PlanInputs& in, cutensorMgContractionPlan* pl) {
    pl->scatterOwners.assign((size_t)(in.nDev * kComputeStreams), {});
    for (const Piece& p : pl->pieces)
        for (const Piece::Scatter& sc : p.scatter) {
            std::vector<int>& v = pl->scatterOwners[(size_t)(p.dev * kComputeStreams + p.stream)];
            for (int o = 0; o < in.nDev; ++o)
                if (o != p.dev && in.h->devices[(size_t)o] == in.d.C.devices[(size_t)sc.cell] && std::find(v.begin(), v.end(), o) == v.end())
                    v.push_back(o);
        }
}

}  // namespace ctamd_mg
