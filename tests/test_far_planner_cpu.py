"""The table of tests/far_cases.py on the CPU planner (no GPU): every case — and every rank it sweeps — plans onto the path it names, sits on
the side of the addressing limit it states (by the table's own span computation), and obeys the three routing rules: no ring kernel on an
operand span of 2^32 - 2^20 bytes or more, no RAG twin on a full span of 2^31 - 2^20 or more, no family-1 plan on a tile span of 2^31 or
more.  The same three rules on a seeded sweep of random far layouts.  Every data draw is checked with the self-checks of tests/exact_data.py
and tests/ew_exact_cases.py (the converting and complex-trinary cases: those of their own tables); nothing here looks at a kernel's result."""
import numpy as np
import pytest

import ew_exact_cases as ew
import exact_cases as xc
import exact_data as xd
import far_cases as fc
import workspace_cases as wc


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", fc.IN_PROCESS)
def test_contraction_case_plans_on_its_path(env, cid):
    ct, ops, h = env
    case = fc.BY_ID[cid]
    ds = fc.plan_paths(ct, ops, h, case)
    if case.sweep:
        assert all(d.get("kname") == case.sweep for d in ds) and len(ds) >= 1
    for swap in (False, True):
        if case.real is None:
            A, B, C = xd.make_exact(case, swap)
            xd.check_draw(case, A, B, C, swap)
        else:                       # (the mixed cases draw with tests/rc64_cases.py: its value set and the fp64 accumulator bound)
            fc.check_rc64_draw(case, *fc.rc.make_inputs(case, swap))


@pytest.mark.parametrize("group", fc.GROUPS)
def test_child_group_plans_on_its_path(built, group):
    cases = [c for c in fc.CASES if c.group == group]
    xc.in_child([c.id for c in cases], cases[0].env, 300, mode="plan", script="far_cases.py")
    for case in cases:
        for swap in (False, True):
            A, B, C = xd.make_exact(case, swap)
            xd.check_draw(case, A, B, C, swap)


@pytest.mark.parametrize("cid", [c.id for c in fc.EW_CASES])
def test_elementwise_case_plans_on_its_path(env, cid):
    ct, ops, h = env
    case = fc.EW_BY_ID[cid]
    d = fc.ew_plan_path(ct, ops, h, case)
    assert 2 <= fc.ew_check_case(case, d) <= ew.MAX_DRAWS
    far, es = case.strides(case.far), fc.ES[case.tdtype(case.far)]
    span = fc.byte_span(case.extents(case.far), far, es)
    assert case.target - (1 << 16) <= span <= case.target and (far[-1] * es) % 16 == 0, (cid, span)
    if case.kind == "reduction" and "farA" in cid:
        kept = case.modes["A"][-1] in case.modes["D"]
        assert cid.endswith("kept" if kept else "reduced")


def test_every_section_of_the_table_names_its_kernels():
    """far_cases.SECTIONS covers every section of both tables (asserted at import), and a full run's launches are checked against it"""
    assert fc.missing_launches([]) == [(sec, w) for sec, ws in fc.SECTIONS.items() for w in ws]
    assert fc.missing_launches([(sec, w + " x", "id") for sec, ws in fc.SECTIONS.items() for w in ws]) == []


def test_the_just_below_cases_reach_the_guarded_kernel():
    """each side of each limit has cases, and the ones below a limit name the kernel the limit guards (their predicates are asserted by the
    tests above): without them the GPU test would have nothing to run"""
    by = {}
    for c in fc.CASES:
        for name, t, rel, limit in c.sides:
            by.setdefault((name, rel, limit), []).append(c)
    ring_below = by[("span", "<", fc.RING_LIMIT)]
    assert all(c.sweep == fc.RING for c in ring_below) and len(ring_below) >= 16
    assert len(by[("span", ">=", fc.RING_LIMIT)]) >= 8
    rag_below = by[("full", "<", fc.RAG_LIMIT)]
    assert all(c.sweep == fc.RING and c.needs_rag() for c in rag_below) and len(rag_below) >= 10
    assert all(not c.sweep and c.needs_rag() for c in by[("full", ">=", fc.RAG_LIMIT)])
    assert len(by[("tile", "<", fc.TILE_LIMIT)]) >= 10 and len(by[("tile", ">=", fc.TILE_LIMIT)]) >= 8


def test_far_strides_reach_the_target_from_below():
    for es in (2, 4, 8, 16):
        for tg in (fc.LO31, fc.HI31, fc.LO32, fc.HI32):
            for ext, pad in (([96, 96], 0), ([37, 9, 7, 2], 3), ([5, 3], 0), ([128, 264], 8)):
                s = fc.far_strides(ext, es, tg, pad)
                span = fc.byte_span(ext, s, es)
                assert span <= tg < span + (ext[-1] - 1) * max(16, es) and (s[-1] * es) % 16 == 0
                assert s[:-1] == fc.padded_strides(ext, pad)[:-1]


# ---- a seeded sweep of random far layouts ----------------------------------------------------------------------------------------------
def _random_case(rng, i):
    dtype = ("float32", "float32", "bfloat16", "float16")[i % 4]
    groups = {"M": "ab", "N": "cd", "K": "kj", "L": "l"}
    use = {g: groups[g][:int(rng.integers(1, 3))] for g in "MNK"}
    use["L"] = "l" if rng.random() < 0.3 else ""
    ext = {}
    for g, ms in use.items():
        for c in ms:
            if g == "K":
                ext[c] = int(rng.choice([32, 64, 100, 128, 8, 25])) if c == "k" else int(rng.choice([2, 3, 4]))
            elif g == "L":
                ext[c] = 2
            else:
                ext[c] = int(rng.choice([8, 12, 16])) if len(ms) == 2 else int(rng.choice([96, 100, 136, 264]))     # (a fused free group stays below 256)
    perm = lambda s: "".join(rng.permutation(list(s)))   # noqa: E731
    mA, mB, mC = perm(use["M"] + use["K"] + use["L"]), perm(use["N"] + use["K"] + use["L"]), perm(use["M"] + use["N"] + use["L"])
    far = "AB"[int(rng.integers(0, 2))]
    target = (fc.LO31, fc.HI31, fc.LO32, fc.HI32)[int(rng.integers(0, 4))]
    quantity = ("full", "span", "tile")[int(rng.integers(0, 3))] if dtype in xd.H16 else ("full", "span")[int(rng.integers(0, 2))]
    if quantity == "tile" and target > fc.HI31:
        target = fc.HI31
    off, align = ((0, None), (0, None), (3, fc.ES[dtype]))[int(rng.integers(0, 3))]
    return fc.FarCase("sweep_%d" % i, dtype, ext, (mA, mB, mC), None, far, target, "sweep", quantity=quantity, off=off, align=align)


def test_random_far_layouts_obey_the_routing_rules(env):
    ct, ops, h = env
    rng = np.random.default_rng(20261020)
    seen = {"ring": 0, "rag": 0, "fam1": 0, "reg": 0, "gen": 0, "plans": 0}
    n = 0
    while n < 200:
        case = _random_case(rng, n)
        # another draw where the slowest mode does not carry the quantity (a batch mode under "span", a mode outside the tile under "tile"),
        # where the packed tensor already passes the target, or where the placed tensor would pass the arena's span
        e, es, t = case.extents(case.tmodes(case.far)), fc.ES[case.dtype], case.far
        packed = fc.padded_strides(e)
        step = packed[:-1] + [packed[-1] + 16 // es]
        q0, q1 = (fc.quantities(case, {t: st})[t][case.quantity] for st in (packed, step))
        if q1 <= q0 or q0 > case.target:
            continue
        if fc.byte_span(e, case.strides(t), es) > (1 << 32) + (1 << 27):
            continue
        q = fc.quantities(case)
        n += 1
        for algo in [None] + (list(range(12)) if case.dtype == "float32" else []):
            try:
                p = fc.make_plan(ct, ops, h, case, algo=algo)
            except ct.CuTensorError:
                break
            try:
                d = wc.describe(ct, p)
            finally:
                p.destroy()
            fc.check_routing(case, d, q)
            seen["plans"] += 1
            seen["ring"] += d.get("kname") == fc.RING
            seen["rag"] += d.get("kname") == fc.RING and case.needs_rag()
            seen["reg"] += d.get("kname") == fc.REG
            seen["fam1"] += d.get("family") == 1
            seen["gen"] += d.get("family") == 2
    print("random far layouts:", seen)
    assert all(seen[k] >= 10 for k in ("ring", "rag", "fam1", "reg", "gen")), seen
