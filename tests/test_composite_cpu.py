"""The table of tests/composite_cases.py on the CPU planner (no GPU): every case plans onto the path it names (or is refused with the status
it names), every draw of every run meets the data rule — the intermediates of all three pair orders of a trinary contraction and every
prefix of a block-sparse output block's contributions are values of the data type, the accumulator bounds hold — and every exact output is
a value of the output type.  All of it is asserted on the data and the references, never on a result of the library.  The references are
compared with the CPU oracle on a few cases, and the table is checked for completeness."""
import numpy as np
import pytest

import composite_cases as cc
from ew_exact_cases import EW_BLOCK, EW_GENERIC, EW_ROWCOPY, EW_TRANSPOSE, EW_TRANSPOSE_ANY

_DESC = {}


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def _describe(env, case):
    if case.id not in _DESC:
        ct, ops, h = env
        _DESC[case.id] = cc.plan_path(ct, ops, h, case)
    return _DESC[case.id]


@pytest.mark.parametrize("case", cc.CASES, ids=[c.id for c in cc.CASES])
def test_case_is_on_its_path_and_its_draws_hold(env, case):
    d = _describe(env, case)
    if case.refuse is not None:
        assert d is None
        return
    assert cc.check_case(case) == 2 * len(case.runs) > 0


def test_the_three_order_cases_report_three_orders(env):
    orders = [tuple(_describe(env, cc.BY_ID["tri_f32_order_" + n])["order"]) for n in ("ab", "ac", "bc")]
    assert orders == [tuple(p) for p in cc.PAIRS]


def test_split_k_steps_put_their_partials_behind_the_intermediate(env):
    for cid, step in (("tri_f32_splitk_step1", "step1"), ("tri_f32_splitk_step2", "step2")):
        d = _describe(env, cc.BY_ID[cid])
        assert d[step]["splitK"] > 1 and d[step]["workspace"] > 0
        assert d["workspace"] == cc.align256(d["intermediate_bytes"]) + max(d["step1"]["workspace"], d["step2"]["workspace"]), d


def test_a_padded_permutation_never_takes_the_unpadded_only_variants(env):
    """EW_BLOCK and EW_TRANSPOSE_ANY are planned for unpadded permutations only: the shapes that take them without padding take another
    variant with it"""
    ct, ops, h = env
    for cid, variant in cc.UNPADDED_TAKES.items():
        plan = cc.make_plan(ct, ops, h, cc.BY_ID[cid], unpadded=True)
        try:
            d = cc.describe(ct, plan)
        finally:
            plan.destroy()
        assert d["variant"] == variant and "pad" not in d, (cid, d)
        assert _describe(env, cc.BY_ID[cid])["variant"] not in (EW_BLOCK, EW_TRANSPOSE_ANY)
    for c in cc.CASES:
        if c.kind == "padded_permutation" and c.refuse is None:
            assert _describe(env, c)["variant"] in (EW_TRANSPOSE, EW_ROWCOPY, EW_GENERIC), c.id


def test_block_sparse_tasks_mirror_the_plan(env):
    """the task list the data rule walks has the plan's length: contributions plus the untouched output blocks"""
    for c in cc.CASES:
        if c.kind == "blocksparse" and c.refuse is None:
            tasks = cc.bs_tasks(c)
            untouched = set(range(len(c.blocks[2]))) - {d for _, _, d in tasks}
            d = _describe(env, c)
            assert d["tasks"] == len(tasks) + len(untouched) and len(untouched) >= 1, (c.id, d)
            counts = sorted({sum(1 for t in tasks if t[2] == b) for b in range(len(c.blocks[2]))})
            assert counts[:3] == [0, 1, 2], (c.id, counts)                                   # no, one and several contributions
            assert len(tasks) < sum(1 for _ in _pairs(c)), c.id                              # a pair whose output block is absent


def _pairs(case):
    mA, mB = case.modes["A"], case.modes["B"]
    for ca in case.blocks[0]:
        for cb in case.blocks[1]:
            sec = dict(zip(mA, ca))
            if all(sec.get(m, x) == x for m, x in zip(mB, cb)):
                yield ca, cb


@pytest.mark.parametrize("cid", ["tri_f32_order_bc", "tri_f64_types", "tri_c64_conj_ABCD", "tri_f32_lone"])
def test_trinary_reference_agrees_with_the_oracle(env, cid):
    """the three-operand einsum as two oracle contractions through an fp64 intermediate (exact on this data in either order)"""
    import oracle
    case = cc.BY_ID[cid]
    ins = cc.make_draw(case, 0)
    m = case.modes
    wide = np.complex128 if case.dtype in cc.CPLX else np.float64
    x = [(np.conj(ins[t]) if t in case.conj else ins[t]).astype(wide) for t in "ABC"]
    mT = "".join(dict.fromkeys(c for c in m["A"] + m["B"] if c in m["C"] or c in m["E"]))
    T = oracle.einsum("%s,%s->%s" % (m["A"], m["B"], mT), x[0], x[1])
    acc = oracle.einsum("%s,%s->%s" % (mT, m["C"], m["E"]), T, x[2])
    for scal, _ in case.runs:
        want = scal[0] * acc + (scal[1] * (np.conj(ins["D"]) if "D" in case.conj else ins["D"]) if scal[1] else 0)
        assert np.array_equal(want, cc.tri_reference(case, ins, scal)), (cid, scal)


def test_the_table_is_complete(env):
    """every pair order; every data type of every entry point; conjugation of each operand on both complex types; every place of the beta
    source per entry point; split-K in either step; a lone-reduce step; the reduced and the fp64-keeping compute descriptors; block-sparse
    in the three layouts with a split-K dense plan; every variant a padded permutation can take, on and off the lane; the refusals"""
    seen = set()
    for c in cc.CASES:
        d = _describe(env, c)
        if c.refuse is not None:
            seen.add(("refused", c.kind, c.dtype))
            continue
        seen.add((c.kind, c.dtype))
        seen |= {(c.kind, "beta", w) for _, w in c.runs}
        if c.kind == "contraction_trinary":
            seen.add(("order", tuple(d["order"])))
            seen |= {("conj", c.dtype, c.conj)} if c.conj else set()
            seen |= {("split", s) for s in ("step1", "step2") if d[s].get("splitK", 1) > 1}
            seen |= {("lone",)} if any(d[s].get("lone_reduce_A") or d[s].get("lone_reduce_B") for s in ("step1", "step2")) else set()
            seen.add(("compute", c.dtype, c.compute, d["step1"]["kname"]))
            seen.add(("layout", bool(c.pad), c.off % 2, c.pad.get("D", 0) != c.pad.get("E", 0)))
        elif c.kind == "blocksparse":
            seen.add(("bs", c.dtype, c.modes["D"], c.layout, d["workspace"] > 0))
        else:
            _, fill, off = cc.pad_geometry(c)
            seen.add(("pp", d["variant"], off % cc.NV[c.dtype] == 0))
            seen.add(("pp_fill", "tiny" if fill * cc.ES[c.dtype] < 16 else "tail" if fill * cc.ES[c.dtype] % 16 else "lanes", c.off % 2))
            seen.add(("pp_value", c.dtype, c.padding[2]))
            seen.add(("pp_op", c.opA))
            left, right, _ = c.padding
            seen.add(("pp_pattern", tuple(bool(x) for x in left), tuple(bool(x) for x in right)))
    want = [("order", tuple(p)) for p in cc.PAIRS] + [(k, dt) for k in ("contraction_trinary", "padded_permutation") for dt in cc.DTYPES]
    want += [("blocksparse", dt) for dt in cc.DTYPES[:4]] + [("refused", "blocksparse", dt) for dt in cc.CPLX + ("float32",)]
    want += [("refused", "padded_permutation", dt) for dt in cc.CPLX]
    want += [(k, "beta", w) for k in ("contraction_trinary", "blocksparse") for w in ("none", "inplace", "separate")]
    want += [("conj", dt, cj) for dt in cc.CPLX for cj in ("A", "B", "C", "D", "ABCD")]
    want += [("split", "step1"), ("split", "step2"), ("lone",)]
    want += [("compute", "float32", cd, "gett_gen_f32x_kernel") for cd in ("16BF", "16F", "TF32")] + [("compute", "float64", "32F", "gett_gen_kernel")]
    want += [("layout", True, 0, True), ("layout", True, 0, False), ("layout", False, 1, False), ("layout", True, 1, False)]
    want += [("bs", dt, mD, lay, False) for dt in cc.DTYPES[:4] for mD in ("i", "il") for lay in ("own", "strided", "packed")]
    want += [("bs", dt, mD, lay, True) for dt in cc.DTYPES[:2] for mD in ("i", "il") for lay in ("own", "packed")]
    want += [("pp", v, lane) for v, lane in ((EW_TRANSPOSE, True), (EW_ROWCOPY, True), (EW_GENERIC, True), (EW_GENERIC, False))]
    want += [("pp_fill", f, o) for f in ("tiny", "tail", "lanes") for o in (0, 1)]
    want += [("pp_value", dt, v) for dt in cc.DTYPES[:4] for v in (7.5, -2.0, float("inf"))] + [("pp_value", dt, None) for dt in cc.CPLX]
    want += [("pp_op", "RELU"), ("pp_pattern", (False,) * 3, (False,) * 3), ("pp_pattern", (True,) * 3, (False,) * 3), ("pp_pattern", (False,) * 3, (True,) * 3),
             ("pp_pattern", (True, False, False), (True, False, False)), ("pp_pattern", (False, False, True), (False, False, True))]
    missing = [w for w in want if w not in seen]
    assert not missing, missing
    assert {cc.pad_value(c) for c in cc.CASES if c.refuse is None and c.padding and isinstance(c.padding[2], bytes)} == {-7.5, 7.5}
    assert any(isinstance(c.padding[2], float) and c.padding[2] == 0.0 and np.signbit(c.padding[2]) for c in cc.CASES if c.kind == "padded_permutation" and c.refuse is None)
    assert len(cc.NO_SWITCH) >= len(cc.RUNNABLE) - 3
