// mg_diagnostics.cpp — entry points of libcutensorMg.so that are not part of the cuTENSORMg ABI (used by the tests and the bench):
// descriptions of the boxes of a ragged contracted mode and of a contraction plan, and the host replay of a plan (hooks flavour only).
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <tuple>

#include "mg_internal.hpp"

using namespace ctamd_mg;

namespace {

// a JSON text under construction
struct Json {
    std::string s;
    template <class... A> void add(const char* fmt, A... a) {
        char tmp[256];
        std::snprintf(tmp, sizeof(tmp), fmt, a...);
        s += tmp;
    }
    template <class V> void list(const char* key, const V& v) {   // "key":[v0,v1,...]
        add("\"%s\":[", key);
        for (size_t i = 0; i < v.size(); ++i) add("%s%lld", i ? "," : "", (long long)v[i]);
        s += "]";
    }
    void lists(const char* key, const std::vector<std::vector<int>>& v) {   // "key":[[..],[..]]
        add("\"%s\":[", key);
        for (size_t i = 0; i < v.size(); ++i) {
            add("%s[", i ? "," : "");
            for (size_t j = 0; j < v[i].size(); ++j) add("%s%d", j ? "," : "", v[i][j]);
            s += "]";
        }
        s += "]";
    }
    void view(const Piece::HostView& hv) { list("extent", hv.extent); s += ","; list("stride", hv.stride); s += ","; list("modes", hv.modes); }
    int copy_out(char* buf, size_t len) const {
        if (s.size() + 1 > len) return -(int)(s.size() + 1);
        std::memcpy(buf, s.c_str(), s.size() + 1);
        return (int)s.size();
    }
};

void describe_piece(Json& j, const Piece& p) {
    j.add("{\"dev\":%d,\"lo\":%lld,\"hi\":%lld,\"lo2\":%lld,\"hi2\":%lld,\"q0\":%lld,\"q1\":%lld,\"stream\":%d,\"flops\":%.6g,\"use\":[", p.dev,
          (long long)p.lo, (long long)p.hi, (long long)p.lo2, (long long)p.hi2, (long long)p.q0, (long long)p.q1, p.stream, p.flops);
    for (int k = 0; k < 3; ++k) {
        j.add("%s{\"direct\":%d,\"off\":%lld,", k ? "," : "", (int)p.use[k].direct, (long long)p.use[k].off);
        j.list("cells", p.use[k].cells);
        j.s += "}";
    }
    j.s += "],";
    j.list("wait", p.waitEvents);
    j.s += ",\"scatter\":[";
    for (size_t c = 0; c < p.scatter.size(); ++c) j.add("%s%d", c ? "," : "", p.scatter[c].cell);
    j.s += "],\"scatterViews\":[";
    for (size_t c = 0; c < p.scatter.size(); ++c) {
        j.add("%s{\"cell\":%d,\"off\":%lld,", c ? "," : "", p.scatter[c].cell, (long long)p.scatter[c].off);
        j.view(p.scatter[c].hv);
        j.s += "}";
    }
    j.s += "],\"subs\":[";
    for (size_t b = 0; b < p.subs.size(); ++b) {
        const Piece::Sub& sub = p.subs[b];
        j.add("%s{\"off\":[%lld,%lld,%lld],\"acc\":%d,\"ws\":%llu,\"views\":[", b ? "," : "", (long long)sub.off[0], (long long)sub.off[1],
              (long long)sub.off[2], (int)sub.accumulate, (unsigned long long)sub.ws);
        for (int k = 0; k < 3; ++k) { j.s += k ? ",{" : "{"; j.view(sub.hv[k]); j.s += "}"; }
        j.s += "]}";
    }
    j.s += "]}";
}

// peeled: digits this plan walks itself; libraryPeeled: local contractions the single-GPU library peels (one tiled inner
// plan launched per index combination); modeTable: local contractions left to the functional mode-table kernel
void describe_local_contractions(Json& j, const cutensorMgContractionPlan* plan) {
    size_t subs = 0, libPeeled = 0, modeTable = 0;
    for (const Piece& p : plan->pieces) {
        subs += p.subs.size();
        for (const Piece::Sub& sub : p.subs) {
            if (ctamdPlanPeelLaunches(sub.plan) > 0) ++libPeeled;
            if (ctamdPlanModeTableGroups(sub.plan, nullptr, nullptr, nullptr, 0) > 0) ++modeTable;
        }
    }
    j.add("{\"peeled\":%d,\"libraryPeeled\":%llu,\"modeTable\":%llu,\"localContractions\":%llu,", plan->peeled, (unsigned long long)libPeeled,
          (unsigned long long)modeTable, (unsigned long long)subs);
}

}  // namespace

extern "C" {

// The boxes kbox_list() cuts the valid part [0, extent) of a padded index space into (block size, digit extents least
// significant first), as JSON: [{"wHi":..,"digits":[[lo,hi],...]},...].
int ctamdMgDescribeKBoxes(int64_t extent, int64_t blockSize, int nDigits, const int64_t* f, char* buf, size_t len) try {
    if (buf == nullptr || len == 0 || blockSize <= 0 || extent <= 0 || nDigits < 0 || (nDigits > 0 && f == nullptr)) return -1;
    Radix r;
    r.blockSize = blockSize;
    r.numBlocks = 1;
    for (int j = 0; j < nDigits; ++j) { r.f.push_back(f[j]); r.numBlocks *= f[j]; }
    if (extent > r.blockSize * r.numBlocks) return -1;
    Json j;
    j.s = "[";
    const std::vector<Clip> boxes = kbox_list(0, r, extent);
    for (size_t i = 0; i < boxes.size(); ++i) {
        j.add("%s{\"wHi\":%lld,\"digits\":[", i ? "," : "", (long long)boxes[i].wHi);
        for (size_t k = 0; k < boxes[i].digit.size(); ++k)
            j.add("%s[%lld,%lld]", k ? "," : "", (long long)boxes[i].digit[k].first, (long long)boxes[i].digit[k].second);
        j.s += "]}";
    }
    j.s += "]";
    return j.copy_out(buf, len);
} CTAMD_API_CATCH_INT

// One JSON object describing the plan: which mode is sharded, the pieces in execution order with the grid cells they
// read in place / from the staging image, their local contractions and scatters with the views, and the events they wait for, the
// size of a device's event block, and every cell transfer.
int ctamdMgDescribePlan(const cutensorMgContractionPlan_t plan, char* buf, size_t len) try {
    if (plan == nullptr || buf == nullptr || len == 0) return -1;
    Json j;
    int64_t remote = 0, local = 0;
    for (const Transfer& t : plan->transfers) (t.local ? local : remote) += t.bytes;
    describe_local_contractions(j, plan);
    j.add("\"numBoxes\":%d,\"allGatherEligible\":[%d,%d],\"transport\":\"%s\",\"trialMs\":[%.4f,%.4f],\"chosen\":%d,", plan->numBoxes,
          (int)plan->allGatherEligible[0], (int)plan->allGatherEligible[1],
          !plan->useRccl ? "peer" : (plan->transport == 2 || !(plan->allGatherEligible[0] || plan->allGatherEligible[1])) ? "sendrecv"
                                    : plan->transport == 1 ? "allgather" : "auto(allgather|sendrecv)",
          plan->trialMs[0], plan->trialMs[1], plan->chosen);
    j.lists("scatterOwners", plan->scatterOwners);
    j.s += ",";
    j.lists("readOwners", plan->readOwners);
    j.s += ",";
    j.add("\"p2Label\":%d,\"forceGather\":%d,", plan->p2Label, (int)plan->forceGather);
    j.add("\"evPerDevice\":%d,\"evScatter\":%d,", plan->ev.perDevice(), plan->ev.scatter_base());
    j.list("usesAux", plan->usesAux); j.s += ","; j.list("usesComm", plan->usesComm); j.s += ",";
    j.add("\"pLabel\":%d,\"qLabel\":%d,\"numWaves\":%d,\"useRccl\":%d,\"commStreams\":%d,\"contractionWs\":%llu,", plan->pLabel, plan->qLabel,
          plan->ev.numWaves, (int)plan->useRccl, plan->ev.commPerDevice, (unsigned long long)plan->contractionWs);
    j.add("\"stagingBytes\":[%lld,%lld,%lld],\"remoteBytes\":%lld,\"localCopyBytes\":%lld,\"pieces\":[", (long long)plan->stagingBytes[0],
          (long long)plan->stagingBytes[1], (long long)plan->stagingBytes[2], (long long)remote, (long long)local);
    for (size_t i = 0; i < plan->pieces.size(); ++i) {
        if (i) j.s += ",";
        describe_piece(j, plan->pieces[i]);
    }
    j.s += "],\"transfers\":[";
    for (size_t i = 0; i < plan->transfers.size(); ++i) {
        const Transfer& t = plan->transfers[i];
        j.add("%s{\"tensor\":%d,\"cell\":%d,\"dst\":%d,\"src\":%d,\"local\":%d,\"wave\":%d,\"bytes\":%lld,\"event\":%d}", i ? "," : "", t.tensor,
              t.cell, t.dst, t.src, (int)t.local, t.wave, (long long)t.bytes, t.event);
    }
    j.s += "]}";
    return j.copy_out(buf, len);
} CTAMD_API_CATCH_INT

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Host replay of a plan (test hook; not part of the cuTENSORMg ABI).  No multi-GPU box is reachable from the build container, so
// the N > 1 data path — which cells travel where, the [cell][cell buffer] staging images, the strided local views, the boxes of
// a ragged contracted mode, peeled digits, the scatter of staged C, and the events a piece waits for — is EXECUTED here over host
// memory instead of only being inspected: A / B / C / D are arrays of HOST cell buffers, every transfer is a memcpy into a host
// staging image, every piece goes through walk_piece — the function cutensorMgContraction executes a piece with — so that every
// local contraction is handed to `contract` (the caller's reference implementation: the tests pass the CPU oracle) on the views,
// offsets, scalars and C / D aliasing the device path hands to cutensorContract, and every scatter is a strided copy between the
// addresses the device path hands to cutensorPermute.  Staging images start as NaN.  Ordering is checked, not simulated: before a
// piece runs, every cell it reads from a staging image must have arrived by a local copy (caller's stream; the auxiliary stream starts
// behind them) or by a transfer whose event the piece's stream has waited for so far — a missing wait is an error even though the
// replay itself is sequential.  Returns 0, or a negative code with a message in `err`.
// ---------------------------------------------------------------------------------------------------------------------
#if CTAMD_HOOKS_BUILT     // compiled into the hooks flavour (lib_hooks/) only: the production library has no test entry points
typedef struct { int32_t n; const int64_t* extent; const int64_t* stride; const int32_t* modes; } ctamdMgHostView;
typedef int (*ctamdMgHostContractFn)(void* user, int dtype, const ctamdMgHostView* A, const void* a, const ctamdMgHostView* B, const void* b,
                                     const ctamdMgHostView* C, const void* c, void* d, double alpha, double beta);

namespace {

// walk_piece over host memory: host cell buffers and host staging images, the test's contraction callback, a strided element copy
struct ReplayBackend {
    const cutensorMgContractionPlan* pl;
    const void* const* src[3];
    void* const* D;
    std::vector<std::vector<std::vector<char>>>& stage;   // [device][tensor]
    ctamdMgHostContractFn contractFn;
    void* user;
    double alpha, beta;

    char* cell(int k, int c) const { return k == 3 ? static_cast<char*>(D[c]) : static_cast<char*>(const_cast<void*>(src[k][c])); }
    char* staging(int g, int k) const { return stage[(size_t)g][(size_t)k].data(); }
    int contract(const Piece&, const Piece::Sub& sub, const char* pa, const char* pb, bool betaIsOne, const char* pc, char* pd) const {
        ctamdMgHostView hv[3];
        for (int k = 0; k < 3; ++k) hv[k] = ctamdMgHostView{(int32_t)sub.hv[k].extent.size(), sub.hv[k].extent.data(), sub.hv[k].stride.data(), sub.hv[k].modes.data()};
        return contractFn(user, (int)pl->desc.A.dtype, &hv[0], pa, &hv[1], pb, &hv[2], pc, pd, alpha, betaIsOne ? 1.0 : beta);
    }
    int scatter(const Piece&, const Piece::Scatter& sc, const char* from, char* to) const {   // identity permutation on strided views
        const int64_t es = (int64_t)elem_size(pl->desc.A.dtype);
        const size_t n = sc.hv.extent.size();
        std::vector<int64_t> idx(n, 0);
        for (;;) {
            int64_t o = 0;
            for (size_t i = 0; i < n; ++i) o += idx[i] * sc.hv.stride[i];
            std::memcpy(to + o * es, from + o * es, (size_t)es);
            size_t i = 0;
            for (; i < n; ++i) {
                if (++idx[i] < sc.hv.extent[i]) break;
                idx[i] = 0;
            }
            if (i == n) return 0;
        }
    }
};

using Arrivals = std::map<std::tuple<int, int, int>, int>;   // (device, tensor, cell) -> event, -1 = local copy

// the gather: every transfer the device path issues (same skip rule for C cells when beta == 0), as a memcpy
int replay_transfers(const ReplayBackend& be, bool betaIsZero, Arrivals* arrivedBy, std::string* msg) {
    for (const Transfer& t : be.pl->transfers) {
        if (skipped_at_beta_zero(t, betaIsZero)) continue;
        if ((size_t)(t.cell + 1) * (size_t)t.bytes > be.stage[(size_t)t.dst][(size_t)t.tensor].size()) { *msg = "a transfer lands outside its staging image"; return -2; }
        if (be.src[t.tensor][t.cell] == nullptr) { *msg = "missing cell buffer"; return -1; }
        std::memcpy(be.staging(t.dst, t.tensor) + (size_t)t.cell * (size_t)t.bytes, be.src[t.tensor][t.cell], (size_t)t.bytes);
        (*arrivedBy)[std::make_tuple(t.dst, t.tensor, t.cell)] = t.local ? -1 : t.event;
    }
    return 0;
}

// the ordering check of one piece: every staged cell it reads has arrived, behind an event its stream has waited for
int check_arrivals(const Piece& p, size_t pi, bool betaIsZero, const Arrivals& arrivedBy, const std::set<int>& waited, std::string* msg) {
    for (int k = 0; k < 3; ++k) {
        if (p.use[k].direct || (k == 2 && betaIsZero)) continue;
        for (int c : p.use[k].cells) {
            const auto it = arrivedBy.find(std::make_tuple(p.dev, k, c));
            if (it == arrivedBy.end()) {
                *msg = "piece " + std::to_string(pi) + " reads a cell nothing transferred (tensor " + std::to_string(k) + ", cell " + std::to_string(c) + ")";
                return -3;
            }
            if (it->second >= 0 && waited.count(it->second) == 0) {
                *msg = "piece " + std::to_string(pi) + " reads tensor " + std::to_string(k) + " cell " + std::to_string(c) + " without having waited for event " + std::to_string(it->second);
                return -4;
            }
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int ctamdMgReplayOnHost(const cutensorMgContractionPlan_t plan, double alpha, const void* const A[], const void* const B[], double beta,
                        const void* const C[], void* const D[], ctamdMgHostContractFn contract, void* user, char* err, size_t errLen) try {
    auto fail = [&](int code, const std::string& msg) {
        if (err != nullptr && errLen > 0) { std::snprintf(err, errLen, "%s", msg.c_str()); }
        return code;
    };
    if (plan == nullptr || A == nullptr || B == nullptr || D == nullptr || contract == nullptr) return fail(-1, "invalid arguments");
    const cutensorMgContractionPlan* pl = plan;
    const int nDev = (int)pl->usesAux.size();
    const bool betaIsZero = beta == 0.0;
    if (!betaIsZero && C == nullptr) return fail(-1, "beta != 0 without C");
    // staging images per device: NaN everywhere (an all-ones bit pattern is a NaN for fp16 / bf16 / fp32 / fp64)
    std::vector<std::vector<std::vector<char>>> stage((size_t)nDev, std::vector<std::vector<char>>(3));
    for (int g = 0; g < nDev; ++g)
        for (int k = 0; k < 3; ++k) stage[(size_t)g][(size_t)k].assign((size_t)pl->stagingBytes[k], (char)0xff);
    ReplayBackend backend{pl, {A, B, C}, D, stage, contract, user, alpha, beta};
    std::string msg;
    Arrivals arrivedBy;
    int rc = replay_transfers(backend, betaIsZero, &arrivedBy, &msg);
    if (rc != 0) return fail(rc, msg);
    // pieces in execution order
    std::vector<std::set<int>> waited((size_t)(nDev * kComputeStreams));
    // fault injection lives HERE, in the checker, never in the plan or the walk a device would execute: with
    // CUTENSORMG_AMD_TEST_DROP_WAITS=1 the replay pretends the pieces wait for nothing (tests/test_mg_replay_cpu.py proves the ordering
    // check live with it)
    const bool dropWaits = CTAMD_HOOK_IS("CUTENSORMG_AMD_TEST_DROP_WAITS", "1");
    for (size_t pi = 0; pi < pl->pieces.size(); ++pi) {
        const Piece& p = pl->pieces[pi];
        std::set<int>& w = waited[(size_t)(p.dev * kComputeStreams + p.stream)];
        if (!dropWaits)
            for (int e : p.waitEvents) w.insert(e);
        rc = check_arrivals(p, pi, betaIsZero, arrivedBy, w, &msg);
        if (rc != 0) return fail(rc, msg);
        if (walk_piece(*pl, p, betaIsZero, backend) != 0) return fail(-5, "the contraction callback failed on piece " + std::to_string(pi));
    }
    return 0;
} CTAMD_API_CATCH_INT

}  // extern "C"
#endif   // CTAMD_HOOKS_BUILT
