"""The case table of the type-converting element-wise tests (tests/test_convert_cpu.py plans every case and checks every draw,
tests/test_gpu_convert_exact.py runs every case) — a helper module, not a conftest.  cutensorPermute and
cutensorElementwiseBinaryExecute with an output (and C) whose data type differs from A's:

    permutation   D = rnd_D(alpha * cmp(perm A))
    binary        D = rnd_D(opAC(alpha * cmp(perm A), gamma * cmp(C)))          C has D's type

for the six pairs bf16 / fp16 -> fp32, fp32 -> bf16 / fp16 (32F, fp32 scalars) and fp32 -> fp64, fp64 -> fp32 (64F, fp64 scalars).

One case is one plan with a predicate on its description: the variant and "convert":[hipDataType of A, of D].  Data, runs, references and
buffers are those of tests/ew_exact_cases.py: integers in [-3, 3], scalars from {+-1, +-2, +-0.5}, every tensor in a NaN-filled buffer
(exact_cases.Placed, with each tensor's own data type) at the case's element offset and padded pitches.  The data is exact in every type,
so the comparison has zero tolerance and says nothing about rounding (tests/test_gpu_convert_rounding.py does); everything outside D's
elements must still be NaN and a separate C must be unchanged.  ew_exact_cases.reference is type-agnostic; expected() is taken in D's
type (Case.dtype is D's type here, Case.dtypeA is A's).

The lane of a pair is LV = 16 / min(sizeof A, sizeof D) elements: 8 for the 16 <-> 32 pairs, 4 for 32 <-> 64.  Shapes per pair:
  * row copy: 'abc -> acb' at a = 32 LV, b = 12, c = 10, packed and with pitches padded by LV / 2 LV on A / D; the binary form with a
    padded C, all four combiners, C in place, apart, and gamma = 0 over a NaN D (ADD).
  * transposition: 'abc -> cba' at a = 17 LV, b = 3, c = 33 LV (interior and edge tiles for a tile of 64, 128 or 256), packed, and padded
    by LV / 2 LV at element offset LV with descriptor alignment 16; the binary form with C in D's layout and once with a C whose fastest
    mode is not D's.  The extent 264 (LV = 8) / 132 (LV = 4) plans 64-wide tiles only, so two more shapes reach the wider tiles: c = 256
    and c = 384 at a = 9 LV (tile0 as the planner's rule gives it: the widest of 256 / 128 / 64 that the extent fills and 32 KiB of LDS
    hold in the parked type — D's when a permutation narrows, else A's).
  * generic: 'abc -> acb' at a = 33, b = 170, c = 7, pitches padded by 1 / 2, element offset 3; 'abc -> cba' at a = 77, b = 5, c = 131
    (an odd transposition says EW_GENERIC, the same-type EW_TRANSPOSE_ANY has no converting twin); a broadcast 'b -> ab', binary.
    Descriptor alignment: each tensor's own element size — the wider element's size for the wider tensor; the narrower tensor at element
    offset 3 is aligned to nothing more than its own size, and cutensorPermute checks each pointer against its descriptor.
  * padding: fp32 -> bf16 on the transposition shape, left / right (1, 0, 2) / (0, 3, 1), pad value -2 (PAD_CASE, run by its own test)."""
import os
import sys

import numpy as np

import ew_exact_cases as ec
import exact_cases as xc
import exact_data as xd
import workspace_cases as wc

PAIRS = (("bfloat16", "float32"), ("float16", "float32"), ("float32", "bfloat16"), ("float32", "float16"), ("float32", "float64"),
         ("float64", "float32"))
SIZE = {"bfloat16": 2, "float16": 2, "float32": 4, "float64": 8}
HIP = {"float32": 0, "float64": 1, "float16": 2, "bfloat16": 14}            # hipDataType values, as ctamdDescribePlan prints them
EW_TRANSPOSE, EW_ROWCOPY, EW_GENERIC = ec.EW_TRANSPOSE, ec.EW_ROWCOPY, ec.EW_GENERIC


def lane(pair):
    return 16 // min(SIZE[pair[0]], SIZE[pair[1]])


def scalar_type(pair):
    """the table's scalar type: fp64 for the 32 <-> 64 pairs, fp32 for the others"""
    return "float64" if "float64" in pair else "float32"


def tile0(pair, binary, e0):
    """the planner's rule for the transposing tile's extent along dim0"""
    narrow = SIZE[pair[1]] < SIZE[pair[0]]
    park = SIZE[pair[1]] if (narrow and not binary) else SIZE[pair[0]]
    cand = min(256, 32768 // (64 * park))
    while cand > 64:
        if e0 % cand == 0 or e0 >= 4 * cand:
            return cand
        cand //= 2
    return 64


class Case(ec.Case):
    """ew_exact_cases.Case with a data type per tensor: dtype is D's (and C's), dtypeA is A's; align may be one number or a dict per tensor"""

    def __init__(self, id, kind, pair, *a, **kw):
        self.pair, self.dtypeA = pair, pair[0]
        ec.Case.__init__(self, id, kind, pair[1], *a, **kw)
        self.data_key = "convert " + self.data_key + pair[0]

    def tdtype(self, t):
        return self.dtypeA if t == "A" else self.dtype

    def alignment(self, t):
        if isinstance(self.align, dict):
            return self.align[t]
        return self.align or 128


CASES = []


def _cv(pair, **want):
    """the description is a plain element-wise one with these values and "convert":[A's type, D's type]"""
    base = ec._is(**want)
    return lambda d: d.get("op") == "elementwise" and d.get("form") is None and d.get("convert") == [HIP[pair[0]], HIP[pair[1]]] and base(d)


def _add(case):
    assert all(case.id != o.id for o in CASES), case.id
    CASES.append(case)


def _name(pair):
    return "%s_%s" % (ec.SHORT[pair[0]], ec.SHORT[pair[1]])


def permutation(name, pair, ext, mA, mD, expect, **kw):
    _add(Case("%s_perm_%s" % (_name(pair), name), "permutation", pair, ext, (mA, mD), expect, [((1.0,), "none"), ((-0.5,), "none")], **kw))


def binary(name, pair, ext, mA, mC, mD, expect, ops=ec.BINOPS, **kw):
    """as ew_exact_cases.binary: C apart; C in place and, for ADD, gamma = 0 over a NaN D where C has D's layout"""
    same = mC == mD and kw.get("pad", {}).get("C", 0) == kw.get("pad", {}).get("D", 0)
    for i, op in enumerate(ops):
        s = ec.EW_SCALARS[(i + len(name)) % 6]
        runs = [((s[0], s[2]), "separate")] + ([((s[1], s[0]), "inplace")] if same else []) + ([((s[2], 0.0), "none")] if op == "ADD" and same else [])
        _add(Case("%s_bin_%s_%s" % (_name(pair), name, op.lower()), "binary", pair, ext, (mA, mC, mD), expect, runs, op=op, **kw))


for _p in PAIRS:
    _lv = lane(_p)
    _own = {"A": SIZE[_p[0]], "C": SIZE[_p[1]], "D": SIZE[_p[1]]}           # each tensor's own element size
    # row copy
    _rc = dict(a=32 * _lv, b=12, c=10)
    permutation("rowcopy", _p, _rc, "abc", "acb", _cv(_p, variant=EW_ROWCOPY, tile0=64 * _lv))
    permutation("rowcopy_pad", _p, _rc, "abc", "acb", _cv(_p, variant=EW_ROWCOPY, tile0=64 * _lv), pad={"A": _lv, "D": 2 * _lv})
    binary("rowcopy_pad", _p, _rc, "abc", "acb", "acb", _cv(_p, variant=EW_ROWCOPY, tile0=64 * _lv), pad={"A": _lv, "C": 2 * _lv, "D": 2 * _lv})
    # transposition: interior and edge tiles
    _tr = dict(a=17 * _lv, b=3, c=33 * _lv)
    permutation("transpose", _p, _tr, "abc", "cba", _cv(_p, variant=EW_TRANSPOSE, tile0=tile0(_p, False, 33 * _lv)))
    permutation("transpose_pad", _p, _tr, "abc", "cba", _cv(_p, variant=EW_TRANSPOSE, tile0=tile0(_p, False, 33 * _lv)), pad={"A": _lv, "D": 2 * _lv},
                off=_lv, align=16)
    binary("transpose", _p, _tr, "abc", "cba", "cba", _cv(_p, variant=EW_TRANSPOSE, tile0=tile0(_p, True, 33 * _lv)))
    binary("transpose_c_order", _p, dict(a=33 * _lv, b=4, c=17 * _lv), "cba", "cab", "abc", _cv(_p, variant=EW_TRANSPOSE), ops=("MUL", "MIN"))
    # the wider tiles
    for _c in (256, 384):
        permutation("transpose_c%d" % _c, _p, dict(a=9 * _lv, b=2, c=_c), "abc", "cba", _cv(_p, variant=EW_TRANSPOSE, tile0=tile0(_p, False, _c)))
    binary("transpose_c256", _p, dict(a=9 * _lv, b=2, c=256), "abc", "cba", "cba", _cv(_p, variant=EW_TRANSPOSE, tile0=tile0(_p, True, 256)), ops=("ADD", "MAX"))
    # generic
    permutation("generic", _p, dict(a=33, b=170, c=7), "abc", "acb", _cv(_p, variant=EW_GENERIC), pad={"A": 1, "D": 2}, off=3, align=_own)
    permutation("generic_odd_transpose", _p, dict(a=77, b=5, c=131), "abc", "cba", _cv(_p, variant=EW_GENERIC))
    binary("generic_pad", _p, dict(a=33, b=34, c=7), "abc", "acb", "acb", _cv(_p, variant=EW_GENERIC), pad={"A": 1, "C": 2, "D": 2}, off=3, align=_own,
           ops=("ADD", "MIN"))
    binary("broadcast", _p, dict(a=20, b=12), "b", "ab", "ab", _cv(_p), ops=("ADD", "MUL"))

BY_ID = {c.id: c for c in CASES}
NO_SWITCH = [c.id for c in CASES if not c.env]

# the padded converting permutation: fp32 -> bf16 on the transposition shape
PAD_PAIR = ("float32", "bfloat16")
PAD_CASE = Case("f32_bf16_perm_transpose_padding", "permutation", PAD_PAIR, dict(a=17 * 8, b=3, c=33 * 8), ("abc", "cba"),
                _cv(PAD_PAIR, variant=EW_GENERIC), [((1.0,), "none"), ((-0.5,), "none")])
PAD_LEFT, PAD_RIGHT, PAD_VALUE = (1, 0, 2), (0, 3, 1), -2.0


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def make_plan(ct, ops, h, case, un=None, padding=None):
    """ops.permutation_plan(dtypeB=) / ops.binary_plan(dtypeC=) where one alignment serves every tensor and C has D's descriptor; else the
    ABI with a descriptor per tensor.  un: unary operators by tensor name (default IDENTITY)."""
    import ctypes
    dA, dD = xc._dt(ct, case.dtypeA), xc._dt(ct, case.dtype)
    m, e, s = case.modes, case.extents, case.strides
    u = {t: ops._unary((un or {}).get(t, "IDENTITY")) for t in "AC"}
    one_align = not isinstance(case.align, dict)
    if case.kind == "permutation" and one_align:
        return ops.permutation_plan(h, e("A"), m["A"], e("D"), m["D"], dtype=dA, dtypeB=dD, strideA=s("A"), strideB=s("D"),
                                    alignment=case.alignment("A"), opA=u["A"], padding=padding)
    if case.kind == "binary" and one_align and m["C"] == m["D"] and s("C") == s("D"):
        return ops.binary_plan(h, e("A"), m["A"], e("D"), m["D"], op=case.op, dtype=dA, dtypeC=dD, alignment=case.alignment("A"), opA=u["A"],
                               opC=u["C"], strideA=s("A"), strideC=s("D"))
    assert padding is None
    desc = {t: ops.tensor_descriptor(h, e(t), s(t), dA if t == "A" else dD, case.alignment(t)) for t in ec.TENSORS[case.kind]}
    opd = ctypes.c_void_p()
    compute = ct.compute_desc(ops._pair_compute(dA, dD))
    if case.kind == "permutation":
        st = ct.cutensorCreatePermutation(h.h, ctypes.byref(opd), desc["A"], ct.i32(m["A"]), u["A"], desc["D"], ct.i32(m["D"]), compute)
    else:
        st = ct.cutensorCreateElementwiseBinary(h.h, ctypes.byref(opd), desc["A"], ct.i32(m["A"]), u["A"], desc["C"], ct.i32(m["C"]), u["C"],
                                                desc["D"], ct.i32(m["D"]), ops._OPS[case.op], compute)
    for d in desc.values():
        ct.cutensorDestroyTensorDescriptor(d)
    ct.check(st)
    return ops.Plan(h, opd, case.kind, dA, workspace_limit=0)


def plan_path(ct, ops, h, case, **kw):
    """the case's plan is on the path the case names (the planner needs no GPU); returns the description"""
    plan = make_plan(ct, ops, h, case, **kw)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d.raw)
        assert plan.scalar_type == xc._dt(ct, scalar_type(case.pair)), (case.id, plan.scalar_type)
        return {k: v for k, v in d.pairs}
    finally:
        plan.destroy()


# ---- running a case ----------------------------------------------------------------------------------------------------------------------
def placed(case, t):
    return xc.Placed(case.extents(t), case.tdtype(t), off=case.off, strides=case.strides(t))


def host(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).reshape(np.shape(x))).to(xd.TORCH_DTYPES[dtype])


def check_case(case):
    """every draw and run of the case on the CPU: the data conditions, and that the reference is exact in D's type AND the inputs in theirs"""
    for draw in range(2):
        ins = ec.make_draw(case, draw, {})
        for t, x in ins.items():
            assert bool((host(x, case.tdtype(t)).to(xd.TORCH_DTYPES["float64"]).numpy() == x).all()), (case.id, t)
        for run in case.runs:
            ec.check_draw(case, ins, run, {})
            ec.expected(case, ec.reference(case, ins, run))


def run_case(ct, ops, h, case):
    import torch
    plan = make_plan(ct, ops, h, case)
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc), "%s is off its path: %s" % (case.id, desc.raw)
        for draw in range(2):
            ins = ec.make_draw(case, draw, {})
            pa = placed(case, "A")
            pa.set(host(ins["A"], case.dtypeA))
            for run in case.runs:
                scal, cmode = run
                ec.check_draw(case, ins, run, {})
                want = ec.expected(case, ec.reference(case, ins, run))
                pd = placed(case, "D")                                     # NaN everywhere
                pc = None
                if cmode == "inplace":
                    pd.set(host(ins["C"], case.dtype))
                elif cmode == "separate":
                    pc = placed(case, "C")
                    pc.set(host(ins["C"], case.dtype))
                if case.kind == "permutation":
                    plan.permute(scal[0], pa.ptr, pd.ptr)
                else:
                    plan.binary(scal[0], pa.ptr, scal[1], pc.ptr if pc else pd.ptr, pd.ptr)
                torch.cuda.synchronize()
                what = "%s (draw %d, scalars %s, C %s) %s" % (case.id, draw, scal, cmode, desc.raw)
                got = pd.get()
                assert got.dtype == xd.TORCH_DTYPES[case.dtype]
                xd.assert_exact(got, want, what)
                pd.check_outside(what)
                pa.check_outside(what + " (A)")
                if pc is not None:
                    xd.assert_exact(pc.get(), host(ins["C"], case.dtype), what + ": C was written")
                    pc.check_outside(what + " (C)")
    finally:
        plan.destroy()


def run_padding(ct, ops, h):
    """PAD_CASE: the output buffer holds extents + left + right per mode, packed; border = the pad value in D's type, interior = alpha * A"""
    import torch
    case = PAD_CASE
    plan = make_plan(ct, ops, h, case, padding=(PAD_LEFT, PAD_RIGHT, PAD_VALUE))
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc), desc.raw
        ins = ec.make_draw(case, 0, {})
        pa = placed(case, "A")
        pa.set(host(ins["A"], case.dtypeA))
        full = [x + l + r for x, l, r in zip(case.extents("D"), PAD_LEFT, PAD_RIGHT)]
        for scal, _ in case.runs:
            ref = ec.reference(case, ins, (scal, "none"))
            want = np.full(full, PAD_VALUE, dtype=np.float64)
            want[tuple(slice(l, l + x) for l, x in zip(PAD_LEFT, case.extents("D")))] = ref
            pd = xc.Placed(full, case.dtype)
            plan.permute(scal[0], pa.ptr, pd.ptr)
            torch.cuda.synchronize()
            what = "%s (alpha %s) %s" % (case.id, scal[0], desc.raw)
            xd.assert_exact(pd.get(), host(want, "float64"), what)
            pd.check_outside(what)
    finally:
        plan.destroy()


if __name__ == "__main__":
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode_ = sys.argv[1]
    if mode_ == "production":
        assert os.environ.get("CTAMD_LIB_FLAVOUR") != "hooks" and "lib_hooks" not in ct_.LIB_PATH, ct_.LIB_PATH
    h_ = ops_.Handle()
    for cid in sys.argv[2:]:
        if mode_ == "plan":
            plan_path(ct_, ops_, h_, BY_ID[cid])
        else:
            run_case(ct_, ops_, h_, BY_ID[cid])
        print("ok", cid, flush=True)
