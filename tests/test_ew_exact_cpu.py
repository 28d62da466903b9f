"""The table of tests/ew_exact_cases.py on the CPU planner (no GPU): every case plans onto the path it names, every draw of every run
satisfies its conditions — accumulator bounds, non-zero reduced elements, the 16-bit exact integer range, MUL exponents, the spike
coverage of MAX / MIN (ends, both sides of every split boundary, the unrolled loops' tails) — and every exact output is a value of the
data type.  All of it is asserted on the data and the references, never on a kernel's result.  The references themselves are compared
with the CPU oracle on a few cases, and the table is checked for completeness: every element-wise variant, every reduction variant with
and without a split, rowAny, 64-bit accumulation of fp32 data and the three trinary forms."""
import numpy as np
import pytest

import ew_exact_cases as ec

_DESC = {}


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def _describe(env, case):
    if case.id not in _DESC:
        ct, ops, h = env
        _DESC[case.id] = ec.plan_path(ct, ops, h, case)
    return _DESC[case.id]


@pytest.mark.parametrize("case", ec.CASES, ids=[c.id for c in ec.CASES])
def test_case_is_on_its_path_and_its_draws_hold(env, case):
    d = _describe(env, case)
    n = ec.check_case(case, d)
    assert 2 <= n <= ec.MAX_DRAWS


def test_forced_positions():
    """a split of 67 rows into 36 + 31: ends, both sides of the boundary, and the 8- / 4- / single-row parts of both splits"""
    pos = ec.forced_positions(67, 2, 36)
    assert {0, 66, 35, 36} <= set(pos)
    assert any(p < 32 for p in pos) and 33 in pos                 # first split: 32 rows by eights, rows 32 .. 35 by four
    assert any(36 <= p < 60 for p in pos) and 61 in pos and 64 in pos     # last split (31 rows): 24 by eights, 60 .. 63 by four, 64 .. 66 singly
    assert ec.forced_positions(5, 1, 8) == [0, 1, 4]


@pytest.mark.parametrize("cid", ["f32_red_col_digits_add", "f32_red_gen_split_max", "f32_red_rowany_mul", "c64_red_gen_split_conjA_add",
                                 "f64_red_col_pad_min", "c128_red_col_odd_split_mul"])
def test_reduction_reference_agrees_with_the_oracle(env, cid):
    import oracle
    case = ec.BY_ID[cid]
    d = _describe(env, case)
    ins = ec.make_draw(case, 0, d)
    wide = np.complex128 if case.dtype in ec.CPLX else np.float64
    op = {"ADD": oracle.OP_ADD, "MUL": oracle.OP_MUL, "MAX": oracle.OP_MAX, "MIN": oracle.OP_MIN}[case.op]
    for run in case.runs:
        (alpha, beta), _ = run
        out = np.zeros(case.extents("D"), dtype=wide)
        oracle.reduce(np.asarray(ins["A"]).astype(wide), case.modes["A"], out, case.modes["D"], alpha=alpha, beta=beta, C=ins["C"].astype(wide), op=op,
                      conjA=case.conjA, conjC=case.conjC)
        assert np.array_equal(out, ec.reference(case, ins, run)), (cid, run)


@pytest.mark.parametrize("cid", ["f32_perm_transpose_t64", "f64_perm_generic", "c64_perm_transpose_conjA", "f32_perm_block_pad"])
def test_permutation_reference_agrees_with_the_oracle(env, cid):
    import oracle
    case = ec.BY_ID[cid]
    ins = ec.make_draw(case, 0, {})
    wide = np.complex128 if case.dtype in ec.CPLX else np.float64
    for run in case.runs:
        out = np.zeros(case.extents("D"), dtype=wide)
        oracle.permute(np.asarray(ins["A"]).astype(wide), case.modes["A"], out, case.modes["D"], alpha=run[0][0], conjA=case.conjA)
        assert np.array_equal(out, ec.reference(case, ins, run)), (cid, run)


def test_the_table_is_complete(env):
    """every EW_* variant (permutation and binary where the planner offers both), every RED_* variant with splitR = 1 and > 1, rowAny with
    and without a split, fp32 accumulated in 64 bits, the three trinary forms each with C in place, and every data type of every kind"""
    seen = set()
    for c in ec.CASES:
        d = _describe(env, c)
        inplace = any(m == "inplace" for _, m in c.runs)
        if c.kind == "reduction":
            seen.add(("red", d["variant"], d["rowAny"], d["splitR"] > 1))
            seen.add(("red", d["variant"], c.dtype, d["splitR"] > 1))
            seen.add(("red_op", d["variant"], d["rowAny"], d["splitR"] > 1, c.op))
            if c.compute == "64F":
                seen.add(("acc64", d["rowAny"], d["splitR"] > 1))
            seen.add(("red_c", ) + tuple(sorted(m for _, m in c.runs)))
        elif c.kind == "trinary":
            seen.add(("tri", d["passes"], d["bothPermuted"], d["swapAB"], inplace))
            seen.add(("tri_dtype", c.dtype, d["passes"]))
        else:
            seen.add((c.kind, d["variant"]))
            seen.add((c.kind, d["variant"], c.dtype))
            if d["variant"] in (ec.EW_TRANSPOSE, ec.EW_TRANSPOSE_ANY):
                seen.add((c.kind, d["variant"], c.dtype in ("bfloat16", "float16"), d["tile0"]))
    want = [("red", v, 0, s) for v in (ec.RED_COL, ec.RED_ROW, ec.RED_GENERIC) for s in (False, True)]
    want += [("red", ec.RED_GENERIC, 1, s) for s in (False, True)] + [("acc64", 0, True), ("acc64", 1, True)]
    want += [("red_op", v, r, s, op) for (v, r) in ((ec.RED_COL, 0), (ec.RED_ROW, 0), (ec.RED_GENERIC, 0), (ec.RED_GENERIC, 1)) for s in (False, True)
             for op in ("ADD", "MUL", "MAX", "MIN")]
    want += [("red", v, dt, s) for v in (ec.RED_COL, ec.RED_ROW) for dt in ec.NV for s in (False, True)]
    want += [("red", ec.RED_GENERIC, dt, True) for dt in ("float32", "float64", "bfloat16", "float16", "complex64")]
    want += [("red_c", "inplace", "none", "separate"), ("red_c", "inplace", "none")]
    want += [("tri", 1, 0, 0, True), ("tri", 1, 0, 1, True), ("tri", 1, 1, 0, True), ("tri", 2, 0, 0, True)]
    want += [("tri_dtype", dt, 2) for dt in ("float32", "float64", "bfloat16", "float16")]
    want += [("permutation", v) for v in range(5)] + [("binary", v) for v in (0, 1, 2, 4)]
    want += [("permutation", ec.EW_TRANSPOSE, False, t) for t in (64, 128, 256)] + [("permutation", ec.EW_TRANSPOSE, True, t) for t in (64, 128, 256)]
    want += [("permutation", ec.EW_TRANSPOSE_ANY, True, 128), ("permutation", ec.EW_TRANSPOSE_ANY, False, 64), ("binary", ec.EW_TRANSPOSE_ANY, False, 64)]
    want += [(k, v, dt) for k in ("permutation", "binary") for v in (ec.EW_TRANSPOSE, ec.EW_ROWCOPY) for dt in ec.NV]
    want += [("permutation", ec.EW_BLOCK, dt) for dt in ("float32", "bfloat16", "float16")]
    missing = [w for w in want if w not in seen]
    assert not missing, missing
    assert len(ec.NO_SWITCH) > 200
