"""Unary operators on element-wise and reduction operands, on the CPU planner (no GPU): which descriptors plan, that an operator never
moves a plan off its identity twin's path, what stays refused, the data tables of tests/test_gpu_unary_exact.py (tests/unary_cases.py),
and the compiled operator twins' resources."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ew_exact_cases as ec
import unary_cases as uc
import workspace_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
_DESC = {}


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


# ---- accepted plans ----------------------------------------------------------------------------------------------------------------------
# one small geometry per entry point (the element-gather kernel's, the tiled kernels' where the type's lane fits)
_SMALL = {"permutation": ("abc", "cba"), "binary": ("abc", "cba", "cba"), "trinary": ("cba", "bac", "abc", "abc"), "reduction": ("abc", "ac")}


@pytest.mark.parametrize("dtype", uc.REAL_DTYPES)
@pytest.mark.parametrize("kind", sorted(_SMALL))
@pytest.mark.parametrize("op", uc.ALL_OPS)
def test_every_operator_plans_on_real_data(env, op, kind, dtype):
    ct, ops, h = env
    base = ec.Case("small", kind, dtype, dict(a=64, b=6, c=16), _SMALL[kind], lambda d: True, [], op=("ADD", "ADD") if kind == "trinary" else "ADD")
    for un in (dict(A=op), dict(C=op), dict(B=op)) if kind == "trinary" else (dict(A=op), dict(C=op)) if kind != "permutation" else (dict(A=op),):
        d = uc.describe(ct, ops, h, base, un)
        codes = [ops._UNARY[un.get(t, "IDENTITY")] for t in "ABC"]
        assert d.get("unary") == codes, (un, d.pairs)
        assert d.get("op") == ("reduction" if kind == "reduction" else "elementwise")


def test_operator_names_and_values(env):
    ct, ops, _ = env
    assert (ct.OP_SQRT, ct.OP_RELU, ct.OP_RCP, ct.OP_SIGMOID, ct.OP_TANH, ct.OP_EXP, ct.OP_LOG, ct.OP_ABS, ct.OP_NEG) == (2, 8, 10, 11, 12, 22, 23, 24, 25)
    assert [ops._unary(n) for n in uc.ALL_OPS] == [ops._UNARY[n] for n in uc.ALL_OPS] and ops._unary("abs") == ct.OP_ABS and ops._unary(ct.OP_NEG) == ct.OP_NEG
    header = open(os.path.join(ROOT, "include", "cutensor", "types.h")).read()
    for name, value in ops._UNARY.items():
        assert re.search(r"CUTENSOR_OP_%s\s*=\s*%d\b" % (name, value), header), name


# ---- the same path as the identity twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", uc.REAL_BASES, ids=[c.id for c in uc.REAL_BASES])
def test_an_operator_keeps_the_identity_plans_path(env, base):
    """every real-data case of the exact table once more with opA = ABS (and opC = NEG where there is a C): the case's own predicate
    holds, and the description equals the identity plan's in every field the latter has — variant, tiles, order, split, workspace"""
    ct, ops, h = env
    un = dict(A="ABS", C="NEG") if base.kind != "permutation" else dict(A="ABS")
    ident = uc.describe(ct, ops, h, base, {})
    with_op = uc.describe(ct, ops, h, base, un)
    assert base.expect(ident) and base.expect(with_op), (ident.pairs, with_op.pairs)
    assert ident.get("unary") is None                                             # today's descriptions stay as they are
    assert list(with_op.pairs[:len(ident.pairs)]) == list(ident.pairs), (ident.pairs, with_op.pairs)
    assert list(with_op.pairs[len(ident.pairs):]) == [("unary", [ct.OP_ABS, ct.OP_IDENTITY, ct.OP_NEG if base.kind != "permutation" else ct.OP_IDENTITY])]


def test_identity_descriptions_are_what_ew_exact_cases_builds(env):
    """the plans this module builds with no operator are the plans of ew_exact_cases.make_plan, byte for byte"""
    ct, ops, h = env
    for base in uc.REAL_BASES[::7]:
        plan = ec.make_plan(ct, ops, h, base)
        try:
            assert wc.describe(ct, plan).pairs == uc.describe(ct, ops, h, base, {}).pairs, base.id
        finally:
            plan.destroy()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _status(ct, fn):
    try:
        fn().destroy()
    except Exception as e:      # ct.check raises with the status in its text
        return str(e)
    return "planned"


def test_refusals(env):
    ct, ops, h = env
    e = [64, 6, 16]
    # complex data takes IDENTITY / CONJ only
    msg = _status(ct, lambda: ops.permutation_plan(h, e, "abc", e[::-1], "cba", dtype=ct.C_32F, opA="SQRT"))
    assert "NOT_SUPPORTED" in msg, msg
    msg = _status(ct, lambda: ops.reduction_plan(h, e, "abc", [64, 16], "ac", dtype=ct.C_32F, opA="SQRT"))
    assert "NOT_SUPPORTED" in msg, msg
    assert _status(ct, lambda: ops.permutation_plan(h, e, "abc", e[::-1], "cba", dtype=ct.C_32F, opA="CONJ")) == "planned"
    # contractions are unchanged
    msg = _status(ct, lambda: ops.contraction_plan(h, [32, 16], "mk", [16, 32], "kn", [32, 32], "mn", opA="SQRT"))
    assert "NOT_SUPPORTED" in msg, msg
    # a unary code where a combiner belongs
    dA, dC = (ops.tensor_descriptor(h, x, None, ct.R_32F, 128) for x in (e, e[::-1]))
    opd = ctypes.c_void_p()
    st = ct.cutensorCreateElementwiseBinary(h.h, ctypes.byref(opd), dA, ct.i32("abc"), ct.OP_IDENTITY, dC, ct.i32("cba"), ct.OP_IDENTITY, dC, ct.i32("cba"),
                                            ct.OP_SQRT, ct.compute_desc("32F"))
    if st == ct.STATUS_SUCCESS:
        msg = _status(ct, lambda: ops.Plan(h, opd, "binary", ct.R_32F, workspace_limit=0))
        assert "NOT_SUPPORTED" in msg, msg
    else:
        assert st == ct.STATUS_NOT_SUPPORTED
    # a combiner where a unary operator belongs
    msg = _status(ct, lambda: ops.permutation_plan(h, e, "abc", e[::-1], "cba", opA=ct.OP_ADD))
    assert "NOT_SUPPORTED" in msg, msg
    for d in (dA, dC):
        ct.cutensorDestroyTensorDescriptor(d)


# ---- the data tables of the exact GPU tests ------------------------------------------------------------------------------------------------
def _describe(env, case):
    if case.id not in _DESC:
        ct, ops, h = env
        _DESC[case.id] = uc.plan_path(ct, ops, h, case)
    return _DESC[case.id]


@pytest.mark.parametrize("case", uc.CASES, ids=[c.id for c in uc.CASES])
def test_case_is_on_its_path_and_its_draws_hold(env, case):
    """on the data and the reference alone: the values each operator meets, the accumulator bound, every exact output a value of the data
    type, the spikes of MAX / MIN at every forced position and decisive only through the operator"""
    d = _describe(env, case)
    n = uc.check_case(case, d)
    assert 2 <= n <= ec.MAX_DRAWS


def test_the_table_is_complete(env):
    """every element-wise variant of real data under operators (permutation and binary), every reduction variant with and without a split
    under each of ABS + MAX, NEG + MIN, RCP + MUL, NEG / RELU + ADD with all three placements of C, the three trinary forms with both values
    of swapAB and the gather launch, every operator of the exact set on every data type"""
    seen = set()
    for c in uc.CASES:
        d = _describe(env, c)
        b = c.base
        for t in "ABC":
            seen.add(("op", c.un[t], b.dtype))
        if b.kind == "reduction":
            seen.add(("red", d["variant"], d["rowAny"], d["splitR"] > 1, b.op, c.un["A"]))
            if b.op == "ADD" and c.un["C"] == "RELU":
                seen.add(("red_c", d["variant"], d["rowAny"], d["splitR"] > 1) + tuple(sorted(m for _, m in b.runs)))
            if b.compute == "64F":
                seen.add(("acc64", d["rowAny"], c.un["A"]))
        elif b.kind == "trinary":
            seen.add(("tri", d["passes"], d["bothPermuted"], d["swapAB"], d["variant_inplace"] >= 0) + tuple(sorted(m for _, m in b.runs)))
        else:
            seen.add((b.kind, d["variant"], b.dtype))
            if d["variant"] in (ec.EW_TRANSPOSE, ec.EW_TRANSPOSE_ANY):
                seen.add((b.kind, d["variant"], b.dtype in ("bfloat16", "float16"), d["tile0"]))
    want = [("op", o, dt) for o in uc.EXACT_OPS for dt in uc.REAL_DTYPES]
    paths = [(v, r, s) for (v, r) in ((ec.RED_COL, 0), (ec.RED_ROW, 0), (ec.RED_GENERIC, 0), (ec.RED_GENERIC, 1)) for s in (False, True)]
    want += [("red", v, r, s, op, u) for (v, r, s) in paths for (op, u) in (("MAX", "ABS"), ("MIN", "NEG"), ("MUL", "RCP"), ("ADD", "NEG"))]
    want += [("red_c", v, r, s, "inplace", "none", "separate") for (v, r, s) in paths]
    want += [("acc64", r, u) for r in (0, 1) for u in ("ABS", "NEG", "RCP")]
    # (two passes: C in a buffer of its own runs both passes, C identical to D the gather launch)
    want += [("tri", 1, 0, 0, False, "inplace", "separate"), ("tri", 1, 0, 1, False, "inplace", "separate"), ("tri", 1, 1, 0, False, "inplace", "separate"),
             ("tri", 2, 0, 0, True, "inplace", "separate")]
    want += [(k, v, dt) for k in ("permutation", "binary") for v in (ec.EW_TRANSPOSE, ec.EW_ROWCOPY, ec.EW_GENERIC) for dt in ("float32", "bfloat16", "float64")]
    want += [("permutation", ec.EW_BLOCK, dt) for dt in ("float32", "bfloat16", "float16")]
    want += [(k, ec.EW_TRANSPOSE_ANY, dt) for k in ("permutation", "binary") for dt in ("float32", "bfloat16", "float16")]
    want += [("permutation", ec.EW_TRANSPOSE, h16, t) for h16 in (False, True) for t in (64, 128, 256)] + [("permutation", ec.EW_TRANSPOSE_ANY, True, 128)]
    missing = [w for w in want if w not in seen]
    assert not missing, missing


def test_reference_agrees_with_a_direct_evaluation(env):
    """the composed reference (operators on the inputs, then the base table's reference) against the formulae written out, on one case
    of each kind"""
    for cid in ("f32_bin_transpose_t64_add", "f32_tri_e_is_b_max_min", "f32_red_col_add", "bf16_red_row_split_max"):
        case = next(c for c in uc.CASES if c.base.id == cid)
        b = case.base
        d = _describe(env, case)
        ins = uc.make_draw(case, 0, d)
        u = {t: uc.PSI[case.un[t]](x) for t, x in ins.items()}
        for run in b.runs:
            s = run[0]
            to = lambda t: ec.to_out(u[t], b.modes[t], b.modes["D"])   # noqa: E731
            if b.kind == "binary":
                want = ec.F[b.op](s[0] * to("A"), s[1] * to("C"))
            elif b.kind == "trinary":
                want = ec.F[b.op[1]](ec.F[b.op[0]](s[0] * to("A"), s[1] * to("B")), s[2] * to("C"))
            else:
                axes = tuple(i for i, c in enumerate(b.modes["A"]) if c not in b.modes["D"])
                want = s[0] * {"ADD": np.sum, "MAX": np.max}[b.op](u["A"], axis=axes) + (s[1] * u["C"] if s[1] else 0.0)
            assert np.array_equal(np.broadcast_to(want, b.extents("D")), uc.reference(case, ins, run)), (cid, run)


# ---- code objects --------------------------------------------------------------------------------------------------------------------------
def _kernel_notes(tmp_path, name):
    """{kernel symbol: {field: int}} of build/obj/<name>.o's gfx950 code object, read as tests/test_kernel_resources.py reads it"""
    obj = os.path.join(ROOT, "build", "obj", name + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no %s or no llvm-objdump in this environment" % obj)
    local = os.path.join(str(tmp_path), name + ".o")
    shutil.copy(obj, local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    co = [f for f in os.listdir(str(tmp_path)) if f.startswith(name + ".o.") and "gfx950" in f]
    assert co, "no gfx950 code object inside %s" % obj
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(str(tmp_path), co[0])], check=True, capture_output=True, text=True).stdout
    kernels, fields, sym = {}, {}, None
    for line in out.splitlines() + ["  - .agpr_count: 0"]:
        if re.match(r"\s*- \.agpr_count:", line):
            if sym is not None:
                kernels[sym] = dict(fields)
            fields, sym = {}, None
        m = re.match(r"\s*\.name:\s+(\S+)", line)
        if m and m.group(1).startswith("_Z"):
            sym = m.group(1)
            continue
        m = re.match(r"\s*(?:- )?\.(private_segment_fixed_size|vgpr_spill_count|vgpr_count|group_segment_fixed_size):\s+(\d+)", line)
        if m:
            fields[m.group(1)] = int(m.group(2))
    return kernels


@pytest.mark.parametrize("obj,twins", [("elementwise", 32), ("reduce", 23)])
def test_operator_twins_use_no_scratch(built, tmp_path, obj, twins):
    """every operator twin (*_un_kernel) comes out with no private segment and no spilled vector register, with the LDS of its identity
    twin, and every identity kernel is still there under its own symbol"""
    k = _kernel_notes(tmp_path, obj)
    un = {n: v for n, v in k.items() if "_un_kernel" in n}
    assert len(un) == twins, sorted(un)
    bad = {n: v for n, v in k.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, bad
    for n, v in un.items():
        twin = re.sub(r"\d+(ew_|reduce_)(\w+?)_un_kernel", lambda m: "%d%s%s_kernel" % (len(m.group(1) + m.group(2)) + 7, m.group(1), m.group(2)), n, count=1)
        assert twin in k, (n, twin)
        assert v.get("group_segment_fixed_size", 0) == k[twin].get("group_segment_fixed_size", 0), (n, v, k[twin])
