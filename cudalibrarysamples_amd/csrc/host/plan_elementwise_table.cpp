// plan_elementwise_table.cpp — the mode-table route of the element-wise family and of cutensorReduce: permutations, binary operations and
// reductions with more unfusable modes than Ew2DParams / ReduceParams describe (two tile modes + four "rest" digits; four kept and four
// reduced digits), up to the 64 modes a tensor descriptor takes.  Kernels: kernels/elementwise_table.hip; the table and its index
// arithmetic: kernels/ew_table_layout.h.
//
// plan_elementwise_any is the one entry: cutensorCreatePermutation / ElementwiseBinary / Reduction, cutensorEstimateWorkspaceSize and
// cutensorCreatePlan (build_elementwise) call it.  It runs today's planner first and takes this route ONLY where that refused the problem
// for its mode count — so every problem that planned before plans exactly as it did — and the route starts from the fused modes that
// planner got as far as (ModeCountRefusal): every other check (labels, extents, operators, data types) has passed by then.
//
// Tile or gather is a question of applicability alone (no time model): the tile kernel where A and D each have a stride-1 mode, A carries
// every mode of D, every stride is positive and a tile spans less than 2^31 elements of each tensor; the gather kernel otherwise, and
// under CUTENSOR_AMD_EW_TABLE=gather (hooks flavour).  A C in another mode order than D stays on the tile kernel: C is read in D's order
// through its own strides.
//
// Still refused with this many modes, as before (each logged under CUTENSOR_LOG_LEVEL): converting pairs, padded permutations
// (build_padded_permutation plans through plan_elementwise) and cutensorCreateElementwiseTrinary (plan_elementwise_trinary does).
#include <algorithm>
#include <cstring>
#include <numeric>

#include "internal.hpp"

namespace ctamd {

bool ew_table_gather_forced() { return CTAMD_HOOK_ENV_IS("CUTENSOR_AMD_EW_TABLE", 'g'); }

namespace {

EwTableMode table_mode(uint32_t count, uint32_t cut, int64_t sA, int64_t sD, int64_t sC) {
    EwTableMode m{};
    m.div = make_fastdiv(count);
    m.cut = cut;
    m.sA = sA; m.sD = sD; m.sC = sC;
    return m;
}

// The tile: take_side walks one side's modes by ascending stride and takes them until their product reaches `target` elements, cutting
// the last one; a mode both sides take gets the longer piece.  tile[i] = 0: mode i is outside the tile.
void take_side(const std::vector<EwMode>& modes, const std::vector<size_t>& order, uint32_t target, std::vector<uint32_t>& tile, uint32_t& taken) {
    uint64_t run = 1;
    taken = 0;
    for (size_t i : order) {
        if (run >= target) break;
        const uint64_t need = (target + run - 1) / run;
        const uint32_t t = (uint32_t)std::min<uint64_t>((uint64_t)modes[i].extent, need);
        tile[i] = std::max(tile[i], t);
        run *= t;
        ++taken;
        if ((int64_t)t < modes[i].extent) break;
    }
}

// true: `tab` describes the tile kernel's launch
bool fill_tile_table(const std::vector<EwMode>& modes, bool usesC, uint32_t elemBytes, EwTable& tab, uint32_t& fromA, uint32_t& fromD) {
    const size_t n = modes.size();
    std::vector<size_t> byD(n), byA(n);
    std::iota(byD.begin(), byD.end(), (size_t)0);                      // (the view is sorted by D's stride)
    byA = byD;
    std::stable_sort(byA.begin(), byA.end(), [&](size_t x, size_t y) { return modes[x].sA < modes[y].sA; });
    for (const EwMode& m : modes)
        if (m.sA <= 0 || m.sD <= 0 || m.sC < 0) return false;           // a mode A lacks (broadcast), or a stride a 32-bit tile offset cannot carry
    if (modes[byD[0]].sD != 1 || modes[byA[0]].sA != 1) return false;   // no stride-1 mode on a side
    // 256-byte runs on both sides; where the union outgrows the tile's positions, A's side halves first, then D's
    const uint32_t cap = ew_table_positions(elemBytes);
    std::vector<uint32_t> tile;
    uint32_t tD = std::max(2u, kEwTableRunBytes / elemBytes), tA = tD;
    uint64_t positions = 0;
    // the tile of a pair of targets; false: more positions than slots, a cut piece too long for its 8-bit digit, or a span beyond 32 bits
    auto build = [&](uint32_t targetD, uint32_t targetA, bool strict) {
        tile.assign(n, 0u);
        take_side(modes, byD, targetD, tile, fromD);
        take_side(modes, byA, targetA, tile, fromA);
        positions = 1;
        uint64_t spanA = 0, spanD = 0, spanC = 0;
        bool fits = true;
        for (size_t i = 0; i < n; ++i) {
            if (tile[i] == 0u) continue;
            positions *= tile[i];
            spanA += (uint64_t)(tile[i] - 1u) * (uint64_t)modes[i].sA;
            spanD += (uint64_t)(tile[i] - 1u) * (uint64_t)modes[i].sD;
            spanC += (uint64_t)(tile[i] - 1u) * (uint64_t)modes[i].sC;
            if ((int64_t)tile[i] < modes[i].extent && tile[i] > 256u) fits = false;
        }
        if (strict && (spanA >= (1ull << 31) || spanD >= (1ull << 31) || spanC >= (1ull << 31))) fits = false;
        return fits && positions <= cap;
    };
    while (!build(tD, tA, false)) {
        if (tA >= tD) tA /= 2; else tD /= 2;                           // (2 x 2 positions always fit)
    }
    // a tile that fits with slots to spare (sets that overlap, modes that are long on one side only) takes longer runs: each side's
    // target doubles, D's side first, as long as the tile still fits
    for (bool grew = true; grew;) {
        grew = false;
        for (int side = 0; side < 2; ++side) {
            const uint64_t had = positions;
            uint32_t& target = side == 0 ? tD : tA;
            const uint32_t before = target;
            bool ok = false;
            for (uint64_t t2 = (uint64_t)before * 2; t2 <= (1ull << 30); t2 *= 2) {
                target = (uint32_t)t2;
                ok = build(tD, tA, true);
                if (!ok || positions > had) break;
            }
            if (ok && positions > had) { grew = true; continue; }
            target = before;
            build(tD, tA, false);
        }
    }
    std::memset(tab.tileA, 0, sizeof(tab.tileA));
    std::memset(tab.tileD, 0, sizeof(tab.tileD));
    std::memset(tab.mode, 0, sizeof(tab.mode));
    tab.cutExtent[0] = tab.cutExtent[1] = 0;
    tab.cutPiece[0] = tab.cutPiece[1] = 0;
    std::vector<uint32_t> cutOf(n, 0u);
    uint32_t nCut = 0, nTile = 0;
    uint64_t spanA = 0, spanD = 0, spanC = 0;
    for (size_t i = 0; i < n; ++i) {
        if (tile[i] == 0u) continue;
        ++nTile;
        spanA += (uint64_t)(tile[i] - 1u) * (uint64_t)modes[i].sA;
        spanD += (uint64_t)(tile[i] - 1u) * (uint64_t)modes[i].sD;
        spanC += (uint64_t)(tile[i] - 1u) * (uint64_t)modes[i].sC;
        if ((int64_t)tile[i] < modes[i].extent) {
            if (nCut == 2u || tile[i] > 256u) return false;
            tab.cutExtent[nCut] = (uint32_t)modes[i].extent;
            tab.cutPiece[nCut] = tile[i];
            cutOf[i] = ++nCut;
        }
    }
    if (nTile > (uint32_t)kEwTableMaxTileModes || spanA >= (1ull << 31) || spanD >= (1ull << 31) || spanC >= (1ull << 31)) return false;
    // the tile's modes in A's order, and what a step of each adds to a position's rank in that order
    std::vector<uint32_t> rankA(n, 0u);
    uint32_t k = 0, rank = 1;
    for (size_t i : byA) {
        if (tile[i] == 0u) continue;
        EwTileMode& m = tab.tileA[k++];
        m.div = make_fastdiv(tile[i]);
        m.cut = cutOf[i];
        m.sA = (uint32_t)modes[i].sA;
        rankA[i] = rank;
        rank *= tile[i];
    }
    tab.nTileA = k;
    k = 0;
    for (size_t i : byD) {
        if (tile[i] == 0u) continue;
        EwTileMode& m = tab.tileD[k++];
        m.div = make_fastdiv(tile[i]);
        m.cut = cutOf[i];
        m.sD = (uint32_t)modes[i].sD;
        m.sC = usesC ? (uint32_t)modes[i].sC : 0u;
        m.rankA = rankA[i];
    }
    tab.nTileD = k;
    tab.tilePos = (uint32_t)positions;
    // the outer index, D's order: the modes outside the tile, and the piece index of each cut mode
    uint64_t tiles = 1;
    k = 0;
    for (size_t i : byD) {
        if (tile[i] != 0u && cutOf[i] == 0u) continue;
        const int64_t step = tile[i] != 0u ? (int64_t)tile[i] : 1;
        const uint64_t count = tile[i] != 0u ? ((uint64_t)modes[i].extent + tile[i] - 1u) / tile[i] : (uint64_t)modes[i].extent;
        tab.mode[k++] = table_mode((uint32_t)count, cutOf[i], modes[i].sA * step, modes[i].sD * step, usesC ? modes[i].sC * step : 0);
        tiles *= count;
        if (tiles >= (1ull << 31)) return false;
    }
    tab.nEntries = k;
    tab.total = (uint32_t)tiles;
    tab.kind = EWT_TILE;
    return true;
}

void fill_gather_table(const std::vector<EwMode>& modes, bool usesC, uint64_t elements, EwTable& tab) {
    std::memset(tab.tileA, 0, sizeof(tab.tileA));
    std::memset(tab.tileD, 0, sizeof(tab.tileD));
    std::memset(tab.mode, 0, sizeof(tab.mode));
    tab.nTileA = tab.nTileD = 0;
    tab.tilePos = 0;
    tab.cutExtent[0] = tab.cutExtent[1] = tab.cutPiece[0] = tab.cutPiece[1] = 0;
    for (size_t i = 0; i < modes.size(); ++i)
        tab.mode[i] = table_mode((uint32_t)modes[i].extent, 0u, modes[i].sA, modes[i].sD, usesC ? modes[i].sC : 0);
    tab.nEntries = (uint32_t)modes.size();
    tab.total = (uint32_t)elements;
    tab.kind = EWT_GATHER;
}

cutensorStatus_t plan_table_elementwise(const cutensorOperationDescriptor& op, const std::vector<EwMode>& modes, int numCUs, EwPlan& plan,
                                        std::string* why) {
    auto fail = [&](const char* msg) {
        if (why) *why = msg;
        return CUTENSOR_STATUS_NOT_SUPPORTED;
    };
    const hipDataType dtype = op.D.desc.dtype;
    if (op.A.desc.dtype != dtype) return fail("too many unfusable modes for a converting plan (the mode-table kernels take one data type)");
    if (op.kind == OpKind::ElementwiseBinary && op.B.present) return fail("too many unfusable modes for a second permuted operand");
    if (modes.size() > (size_t)kEwTableMaxModes) return fail("too many unfusable modes");
    uint64_t elements = 1;
    for (const EwMode& m : modes) {
        elements *= (uint64_t)m.extent;
        if (elements >= (1ull << 31)) return fail("tensor too large for the tile index space");
    }
    const bool usesC = op.C.present;
    const bool cplx = dtype == HIP_C_32F || dtype == HIP_C_64F;
    auto tab = std::make_shared<EwTable>();
    std::memset(tab.get(), 0, sizeof(EwTable));
    tab->opAC = op.kind == OpKind::ElementwiseBinary ? (int32_t)op.opReduce : (int32_t)CUTENSOR_OP_ADD;   // (every other caller adds)
    tab->opReduce = (int32_t)CUTENSOR_OP_ADD;
    tab->conjA = (cplx && op.A.op == CUTENSOR_OP_CONJ) ? 1 : 0;
    tab->conjC = (cplx && usesC && op.C.op == CUTENSOR_OP_CONJ) ? 1 : 0;
    tab->unA = (uint8_t)unary_code(op.A.op);
    tab->unC = usesC ? (uint8_t)unary_code(op.C.op) : (uint8_t)0;
    tab->nModes = (uint32_t)modes.size();
    const uint32_t es = (uint32_t)dtype_size(dtype);
    uint32_t fromA = 0, fromD = 0;
    const bool tiled = !ew_table_gather_forced() && !modes.empty() && fill_tile_table(modes, usesC, es, *tab, fromA, fromD);
    if (!tiled) fill_gather_table(modes, usesC, elements, *tab);
    plan = EwPlan{};
    plan.usesC = usesC;
    plan.variant = tiled ? EW_TABLE_TILE : EW_TABLE_GATHER;
    plan.dtypeA = plan.dtypeD = dtype;
    // what the description and reads_c (exec_elementwise.cpp) read from the 2-D block
    plan.p.opAC = op.kind == OpKind::ElementwiseBinary ? (int32_t)op.opReduce : 0;
    plan.p.unA = tab->unA; plan.p.unC = tab->unC;
    plan.p.conjA = tab->conjA; plan.p.conjC = tab->conjC;
    plan.p.nBlocks = tab->total;
    plan.tabFromA = tiled ? fromA : 0u;
    plan.tabFromD = tiled ? fromD : 0u;
    // a grid sized by the device, each workgroup looping over tiles / elements (as the persistent kernels): four workgroups a CU — and, on
    // the tile kernel, no more workgroups than a quarter of the tiles: a workgroup builds its table of tile-relative offsets once (two
    // mixed-radix decodes per position, more work than moving a tile) and should have a few tiles to spread that over
    uint64_t units = (elements + kEwTableThreads - 1) / kEwTableThreads;
    if (tiled) units = ((uint64_t)tab->total + 3u) / 4u;
    plan.tabGrid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(units, (uint64_t)std::max(numCUs, 1) * 4u));
    plan.tab = std::move(tab);
    return CUTENSOR_STATUS_SUCCESS;
}

cutensorStatus_t plan_table_reduction(const cutensorOperationDescriptor& op, std::vector<EwMode> kept, const std::vector<EwMode>& red, uint64_t wsLimit,
                                      int numCUs, ReducePlan& plan, std::string* why) {
    auto fail = [&](const char* msg) {
        if (why) *why = msg;
        return CUTENSOR_STATUS_NOT_SUPPORTED;
    };
    if (kept.size() + red.size() > (size_t)kEwTableMaxModes) return fail("mode group too large");
    // a lane per kept element in D's order
    std::stable_sort(kept.begin(), kept.end(), [](const EwMode& x, const EwMode& y) { return x.sD < y.sD; });
    uint64_t keptTot = 1, redTot = 1;
    for (const EwMode& m : kept) { keptTot *= (uint64_t)m.extent; if (keptTot >= (1ull << 31)) return fail("mode group too large"); }
    for (const EwMode& m : red)  { redTot *= (uint64_t)m.extent;  if (redTot >= (1ull << 31)) return fail("mode group too large"); }
    const hipDataType dtype = op.A.desc.dtype;
    const bool cplx = dtype == HIP_C_32F || dtype == HIP_C_64F;
    auto tab = std::make_shared<EwTable>();
    std::memset(tab.get(), 0, sizeof(EwTable));
    tab->kind = EWT_REDUCE;
    tab->opAC = (int32_t)CUTENSOR_OP_ADD;
    tab->opReduce = (int32_t)op.opReduce;
    tab->conjA = (cplx && op.A.op == CUTENSOR_OP_CONJ) ? 1 : 0;
    tab->conjC = (cplx && op.C.op == CUTENSOR_OP_CONJ) ? 1 : 0;
    tab->unA = (uint8_t)unary_code(op.A.op);
    tab->unC = (uint8_t)unary_code(op.C.op);
    tab->nModes = (uint32_t)(kept.size() + red.size());
    tab->nEntries = tab->nModes;
    tab->nKept = (uint32_t)kept.size();
    tab->nRed = (uint32_t)red.size();
    tab->total = (uint32_t)keptTot;
    tab->redTotal = (uint32_t)redTot;
    uint32_t k = 0;
    for (const EwMode& m : kept) tab->mode[k++] = table_mode((uint32_t)m.extent, 0u, m.sA, m.sD, m.sC);
    for (const EwMode& m : red)  tab->mode[k++] = table_mode((uint32_t)m.extent, 0u, m.sA, 0, 0);
    // the split of the reduced range: RED_GENERIC's rule (plan_reduction) — a lane per kept element wants numCUs * 512 of them
    const bool acc64 = (op.compute != nullptr && op.compute->id == 5 /*64F*/) || dtype == HIP_R_64F;
    const uint64_t accBytes = dtype == HIP_C_64F ? 16 : dtype == HIP_C_32F ? 8 : (acc64 ? 8 : 4);
    const uint64_t wantItems = (uint64_t)numCUs * 512, minRedPerSplit = 64, gran = 4;
    uint64_t split = 1;
    if (keptTot < wantItems) split = (wantItems + keptTot - 1) / keptTot;
    split = std::min<uint64_t>(split, std::max<uint64_t>(redTot / minRedPerSplit, 1));
    split = std::min<uint64_t>(split, 4096);
    while (split > 1 && split * keptTot * accBytes > wsLimit) split /= 2;
    uint64_t per = (redTot + split - 1) / split;
    per = ((per + gran - 1) / gran) * gran;
    split = (redTot + per - 1) / per;
    tab->splitR = (uint32_t)std::max<uint64_t>(split, 1);
    tab->redPerSplit = (uint32_t)per;
    plan = ReducePlan{};
    plan.variant = RED_TABLE;
    std::memset(&plan.p, 0, sizeof(plan.p));
    plan.p.kept.total = tab->total;
    plan.p.red.total = tab->redTotal;
    plan.p.splitR = tab->splitR;
    plan.p.redPerSplit = tab->redPerSplit;
    plan.p.op = tab->opReduce;
    plan.p.unA = tab->unA; plan.p.unC = tab->unC;
    plan.p.conjA = tab->conjA; plan.p.conjC = tab->conjC;
    plan.workspace = tab->splitR > 1 ? (uint64_t)tab->splitR * keptTot * accBytes : 0;
    plan.tab = std::move(tab);
    return CUTENSOR_STATUS_SUCCESS;
}

}  // namespace

cutensorStatus_t plan_elementwise_any(const cutensorOperationDescriptor& op, uint64_t wsLimit, int numCUs, EwPlan& ew, ReducePlan& red,
                                      std::string* why) {
    ModeCountRefusal over;
    if (op.kind == OpKind::Reduction) {
        const cutensorStatus_t st = plan_reduction(op, wsLimit, numCUs, red, why, &over);
        if (st != CUTENSOR_STATUS_NOT_SUPPORTED || !over.hit) return st;
        if (!red.isPermutation) return plan_table_reduction(op, over.kept, over.red, wsLimit, numCUs, red, why);
        // no reduced mode: D = alpha perm(A) + beta C, the binary form (plan_reduction's own rewrite)
        cutensorOperationDescriptor e = op;
        e.kind = OpKind::ElementwiseBinary;
        e.opReduce = CUTENSOR_OP_ADD;
        e.C.present = true;
        return plan_table_elementwise(e, over.modes, numCUs, red.perm, why);
    }
    const cutensorStatus_t st = plan_elementwise(op, ew, why, true, &over);
    if (st != CUTENSOR_STATUS_NOT_SUPPORTED || !over.hit) return st;
    return plan_table_elementwise(op, over.modes, numCUs, ew, why);
}

}  // namespace ctamd
