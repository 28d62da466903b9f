"""Element-wise trinary operations on complex data, on the CPU planner (no GPU; the table is tests/cplx_trinary_cases.py): every case plans
onto the path it names with complex scalars of the data's type, every draw is exact on the reference, the refusals the interface documents
are CUTENSOR_STATUS_NOT_SUPPORTED, CONJ on a real descriptor is the identity, and real-data trinary planning is where it was before the
complex kernels arrived (tests/golden/trinary_real_descriptions.json, written by tools/gen_trinary_real_descriptions.py on the commit
before them)."""
import ctypes
import json
import os

import pytest

import cplx_trinary_cases as tc
import ew_exact_cases as ec
import workspace_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trinary_real_descriptions.json")


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("case", tc.CASES, ids=[c.id for c in tc.CASES])
def test_case_is_on_its_path_and_its_draws_hold(env, case):
    ct, ops, h = env
    d = tc.plan_path(ct, ops, h, case)
    assert d["conj"] == [int(c) for c in case.conj3]
    tc.check_case(case)


def test_the_table_reaches_every_form_with_every_combiner_rule():
    for dt in tc.DTYPES:
        mine = [c for c in tc.CASES if c.dtype == dt]
        for form, is_form in tc.FORMS.items():
            ops_ = {c.op for c in mine if is_form(c)}
            assert ("MUL", "MUL") in ops_, (dt, form, ops_)
        assert {c.op for c in mine} == set(tc.COMBINERS), dt
        # gamma = 0 over a NaN C, the in-place launch of the two-pass form, C apart
        assert any(r[1] == "none" for c in mine for r in c.runs) and any(r[1] == "inplace" and "two_pass" in c.id for c in mine for r in c.runs)
        # conjugation: each operand alone and all three, on the E, two-tile and row-copy forms
        for form in ("e_is_a", "two_tiles", "rowcopy"):
            assert {c.conj3 for c in mine if any("_%s_%s_" % (form, k) in c.id for k in tc.CONJ)} == set(tc.CONJ.values()), (dt, form)
    gather = [c for c in tc.CASES if "gather" in c.id]
    assert gather and all(c.dtype == "complex64" and c.off == 1 and c.align == 8 for c in gather)


def _status(fn):
    try:
        fn().destroy()
    except Exception as e:                                                     # ct.check raises with the status name
        return str(e)
    return "SUCCESS"


E, ED = [16, 8, 24], [24, 8, 16]


def _tri(env, dtype="C_32F", **kw):
    ct, ops, h = env
    return lambda: ops.trinary_plan(h, E, "abc", ED, "cba", ED, "cba", ED, "cba", dtype=getattr(ct, dtype), **kw)


@pytest.mark.parametrize("dtype", ("C_32F", "C_64F"))
def test_refusals_on_complex_data(env, dtype):
    ct = env[0]
    assert _status(_tri(env, dtype)) == "SUCCESS"
    assert _status(_tri(env, dtype, opA="CONJ", opB="CONJ", opC="CONJ", opAB="MUL", opABC="MUL")) == "SUCCESS"
    for bad in ("MAX", "MIN"):
        assert "NOT_SUPPORTED" in _status(_tri(env, dtype, opAB=bad)), bad
        assert "NOT_SUPPORTED" in _status(_tri(env, dtype, opABC=bad)), bad
    for un in ("SQRT", "RELU", "RCP", "SIGMOID", "TANH", "EXP", "LOG", "ABS", "NEG"):
        for which in ("opA", "opB", "opC"):
            assert "NOT_SUPPORTED" in _status(_tri(env, dtype, **{which: un})), (which, un)


def test_mixed_data_types_stay_refused(env):
    ct, ops, h = env
    T = {"f32": ct.R_32F, "f64": ct.R_64F, "c64": ct.C_32F, "c128": ct.C_64F}

    def tri(ta, tb, tc_, td):
        d = [ops.tensor_descriptor(h, E, None, T[ta]), ops.tensor_descriptor(h, ED, None, T[tb]), ops.tensor_descriptor(h, ED, None, T[tc_]),
             ops.tensor_descriptor(h, ED, None, T[td])]
        opd = ctypes.c_void_p()
        st = ct.cutensorCreateElementwiseTrinary(h.h, ctypes.byref(opd), d[0], ct.i32("abc"), ct.OP_IDENTITY, d[1], ct.i32("cba"), ct.OP_IDENTITY, d[2],
                                                 ct.i32("cba"), ct.OP_IDENTITY, d[3], ct.i32("cba"), ct.OP_ADD, ct.OP_ADD, ct.compute_desc("32F"))
        for x in d:
            ct.cutensorDestroyTensorDescriptor(x)
        ct.check(st)
        return ops.Plan(h, opd, "trinary", T[ta], workspace_limit=0)
    assert _status(lambda: tri("c64", "c64", "c64", "c64")) == "SUCCESS"
    for mix in (("c64", "c64", "c64", "c128"), ("c128", "c64", "c64", "c64"), ("c64", "c128", "c64", "c64"), ("c64", "c64", "c128", "c64"),
                ("f32", "c64", "c64", "c64"), ("c64", "f32", "c64", "c64"), ("c64", "c64", "f32", "c64"), ("c64", "c64", "c64", "f32"),
                ("f64", "f64", "f64", "c128"), ("c128", "c128", "c128", "f64")):
        assert "NOT_SUPPORTED" in _status(lambda: tri(*mix)), mix


@pytest.mark.parametrize("dtype", ("R_32F", "R_64F", "R_16BF", "R_16F"))
def test_conj_on_a_real_descriptor_is_the_identity(env, dtype):
    ct = env[0]

    def raw(**kw):
        p = _tri(env, dtype, **kw)()
        try:
            return wc.describe(ct, p).raw
        finally:
            p.destroy()
    plain = raw()
    assert plain and '"conj"' not in plain and '"unary"' not in plain
    for kw in (dict(opA="CONJ"), dict(opB="CONJ"), dict(opC="CONJ"), dict(opA="CONJ", opB="CONJ", opC="CONJ")):
        assert raw(**kw) == plain, kw
    # beside another operand's operator too
    assert raw(opA="CONJ", opB="ABS") == raw(opB="ABS") != plain


def test_scalar_type_and_moved_bytes(env):
    ct, ops, h = env
    for dtype, size in ((ct.C_32F, 8), (ct.C_64F, 16)):
        p = ops.trinary_plan(h, E, "abc", ED, "cba", ED, "cba", ED, "cba", dtype=dtype, opA="CONJ")
        moved, st = ctypes.c_float(0), ctypes.c_int(-1)
        ct.check(ct.cutensorOperationDescriptorGetAttribute(h.h, p.op, ct.OPERATION_DESCRIPTOR_MOVED_BYTES, ctypes.byref(moved), 4))
        ct.check(ct.cutensorOperationDescriptorGetAttribute(h.h, p.op, ct.OPERATION_DESCRIPTOR_SCALAR_TYPE, ctypes.byref(st), 4))
        assert moved.value == float(4 * 16 * 8 * 24 * size) and st.value == dtype == p.scalar_type
        assert len(p.scalar(1 + 2j)) == 2
        p.destroy()


def test_real_data_trinary_descriptions_are_unchanged(env):
    """every real-data trinary case of ew_exact_cases.CASES describes byte for byte as on the commit before the complex kernels"""
    ct, ops, h = env
    with open(GOLDEN) as f:
        golden = json.load(f)
    cases = [c for c in ec.CASES if c.kind == "trinary" and c.dtype not in ec.CPLX]
    assert cases and sorted(c.id for c in cases) == sorted(golden)
    for c in cases:
        plan = ec.make_plan(ct, ops, h, c)
        try:
            assert wc.describe(ct, plan).raw == golden[c.id], c.id
        finally:
            plan.destroy()
