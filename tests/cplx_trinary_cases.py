"""The case table of the complex element-wise trinary tests (tests/test_cplx_trinary_cpu.py plans every case and checks every draw,
tests/test_gpu_cplx_trinary_exact.py runs every case) — a helper module, not a conftest, built on ew_exact_cases.Case and
exact_cases.Placed the way tests/convert_cases.py is.

    D = opABC(opAB(alpha * cjA(perm A), beta * cjB(perm B)), gamma * cjC(perm C))      on complex64 / complex128 tensors,

cj = identity or conjugation per operand, opAB / opABC = ADD or MUL, complex scalars (kernels/elementwise_trinary_cplx.hip).

One case is one plan with a predicate on its description: the form fields (passes, bothPermuted, swapAB), the variants and "conj".  Data:
both parts of every element an integer in [-3, 3] (ew_exact_cases.make_draw), both parts of every scalar from {0, +-1, +-2, +-0.5}, and in
every run at least one scalar with two non-zero parts.  Every tensor sits in a NaN-filled buffer (exact_cases.Placed) at the case's
element offset and padded pitches; after each launch D is compared with zero tolerance, everything outside D's elements must still be
NaN, and A, B and a separate C must be unchanged.  Runs: C in a buffer of its own ("separate"), C identical to D ("inplace": in the two-pass
form that is the single launch the description calls variant_inplace) and, where opABC is ADD and C has D's layout, gamma = 0 with D — which
is also passed as C — full of NaN ("none": C must not be read).

Exactness: alpha * a has parts of magnitude <= 12 at granularity 1/2, a product of two such terms <= 288 at 1/4, the product of that with
a third <= 6912 at 1/8.  So every intermediate — each scaled operand, opAB's result, the output — is a dyadic rational below 2^14 at
granularity 1/8: 17 binary digits, exact in fp32 in any order of the four real products and two sums of a complex product.  reference()
asserts exactly that on every intermediate it forms.

Shapes (the smallest that reach interior and edge tiles; a 16-byte lane holds NV = 2 complex64 / 1 complex128 elements, the transposing tile
is 128 x 32 / 64 x 32, and 64 x 64 for complex64 with a second tile):
  * E = A and E = B: 'abc, cab -> abc' and the swap at a = 130, b = 3, c = 66; once with a C laid out 'bca' (b has stride 1 there: odd
    beside complex64's 2-element lanes, so that type plans the gather kernel) and once 'cba' (tiled, C read element by element).
  * row copy with E: 'abc, acb -> abc' at a = 256, b = 12, c = 10, packed and with padded pitches.
  * two tiles: 'cba, cab -> abc' at a = 130, b = 4, c = 66, packed and padded.
  * two passes: 'cba, bac -> abc' at (68, 34, 12) — tiled on both types — and at (68, 33, 12), where the last pass of complex64 falls to
    the gather kernel (an odd extent along B's stride-1 mode) and complex128 stays tiled.  With C identical to D the single gather launch
    runs: the only way to ew3c_generic_kernel on complex128 data, whose 16-byte descriptors are otherwise always tiled.
  * gather: complex64 at (33, 7, 5), element offset 1, descriptor alignment 8: the E form and the two-pass form.
  * conjugation of A, B, C alone and of all three, in every role an operand can take: tile operand, E, X (second tile, and the gather
    kernel's X), C, and pass 1 of the two-pass form.  check_case asserts that the reference without the conjugation differs.
Per form (MUL, MUL) runs at least once per type; the other cases rotate through (ADD, ADD), (MUL, ADD), (ADD, MUL), (MUL, MUL)."""
import os
import sys

import numpy as np

import ew_exact_cases as ec
import exact_cases as xc
import exact_data as xd
import workspace_cases as wc

DTYPES = ("complex64", "complex128")
COMBINERS = (("ADD", "ADD"), ("MUL", "ADD"), ("ADD", "MUL"), ("MUL", "MUL"))
EW_TRANSPOSE, EW_ROWCOPY, EW_GENERIC = ec.EW_TRANSPOSE, ec.EW_ROWCOPY, ec.EW_GENERIC
NV = ec.NV
TILE0 = {"complex64": 128, "complex128": 64}
# (alpha, beta, gamma): parts from {0, +-1, +-2, +-0.5}; every triple holds a scalar with two non-zero parts
SCALARS = [(1 + 2j, 0.5 - 1j, -1 + 0.5j), (-2 + 0.5j, 1j, 2 - 1j), (0.5 + 0.5j, -1 - 2j, 1.0), (-1j, 2 + 1j, -0.5 + 2j), (2.0, -0.5 + 1j, 1 - 1j),
           (-0.5 - 2j, 1.0, 0.5j)]
PARTS = (0.0, 1.0, 2.0, 0.5)
LIMIT, GRAIN = 2.0 ** 14, 8.0


class Case(ec.Case):
    """ew_exact_cases.Case of kind "trinary" with a conjugation flag per operand (A, B, C)"""

    def __init__(self, id, dtype, ext, modes, expect, runs, op, conj3=(False, False, False), **kw):
        ec.Case.__init__(self, id, "trinary", dtype, ext, modes, expect, runs, op=op, **kw)
        self.conj3 = tuple(bool(c) for c in conj3)
        self.data_key = "cplx trinary " + self.data_key


CASES = []
_COUNT = {}


def _want(conj3=(False, False, False), **want):
    base = ec._is(**want)
    return lambda d: d.get("op") == "elementwise" and d.get("form") == "trinary" and d.get("conj") == [int(c) for c in conj3] and base(d)


def tri(name, dtype, ext, modes, want, ops=None, conj3=(False, False, False), n=1, cmodes=("separate", "inplace"), **kw):
    """one case per combiner pair: `ops`, or the next n pairs of the type's rotation"""
    mC, mD = modes[2], modes[3]
    same = mC == mD and kw.get("pad", {}).get("C", 0) == kw.get("pad", {}).get("D", 0)
    cid = lambda op: "%s_tri_%s_%s_%s" % (ec.SHORT[dtype], name, op[0].lower(), op[1].lower())   # noqa: E731
    if ops is None:
        ops = []
        while len(ops) < n:                                    # (a pair the name already ran with is passed over)
            k = _COUNT.get(dtype, 0)
            _COUNT[dtype] = k + 1
            if all(cid(COMBINERS[k % 4]) != o.id for o in CASES) and COMBINERS[k % 4] not in ops:
                ops.append(COMBINERS[k % 4])
    for i, op in enumerate(ops):
        s = [SCALARS[(i + len(name) + j) % 6] for j in range(3)]
        runs = [(s[0], "separate")] if "separate" in cmodes else []
        if same and "inplace" in cmodes:
            runs.append((s[1], "inplace"))
        if same and op[1] == "ADD":
            runs.append(((s[2][0], s[2][1], 0.0), "none"))
        c = Case(cid(op), dtype, ext, modes, _want(conj3, **want), runs, op, conj3, **kw)
        assert all(c.id != o.id for o in CASES), c.id
        CASES.append(c)


MM = [("MUL", "MUL")]
CONJ = {"cA": (True, False, False), "cB": (False, True, False), "cC": (False, False, True), "cABC": (True, True, True)}
for _dt in DTYPES:
    _nv, _t0 = NV[_dt], TILE0[_dt]
    _e = dict(a=130, b=3, c=66)
    _one = dict(passes=1, bothPermuted=0, variant=EW_TRANSPOSE, tile0=_t0, variant_first=-1, variant_inplace=-1)
    # E = A, E = B; a C whose stride-1 mode is not D's
    tri("e_is_a", _dt, _e, ("abc", "cab", "abc", "abc"), dict(_one, swapAB=0), ops=COMBINERS)
    tri("e_is_b", _dt, _e, ("cab", "abc", "abc", "abc"), dict(_one, swapAB=1), ops=MM)
    tri("e_is_b", _dt, _e, ("cab", "abc", "abc", "abc"), dict(_one, swapAB=1), n=1)
    # (C laid out 'bca': b has stride 1 in C — an odd stride beside complex64's 2-element lanes, so that type plans the gather kernel;
    # 'cba' keeps every stride of C even and the tiles, and C is read element by element along dim0)
    tri("e_is_a_c_bca", _dt, _e, ("abc", "cab", "bca", "abc"), dict(_one, swapAB=0, **(dict(variant=EW_GENERIC, tile0=64) if _dt == "complex64" else {})), n=1)
    tri("e_is_a_c_cba", _dt, _e, ("abc", "cab", "cba", "abc"), dict(_one, swapAB=0), n=1)
    tri("e_is_a_c_cba_cC", _dt, _e, ("abc", "cab", "cba", "abc"), dict(_one, swapAB=0), conj3=(False, False, True), n=1)
    # row copy with E
    _r = dict(a=256, b=12, c=10)
    _row = dict(passes=1, bothPermuted=0, swapAB=0, variant=EW_ROWCOPY, tile0=64 * _nv)
    tri("rowcopy", _dt, _r, ("abc", "acb", "abc", "abc"), _row, ops=MM)
    tri("rowcopy", _dt, _r, ("abc", "acb", "abc", "abc"), _row, n=1)
    tri("rowcopy_pad", _dt, _r, ("abc", "acb", "abc", "abc"), _row, n=2, pad={"A": 2, "B": 4, "C": 2, "D": 2})
    # two tiles
    _t = dict(a=130, b=4, c=66)
    _two = dict(passes=1, bothPermuted=1, swapAB=0, variant=EW_TRANSPOSE, tile0=64)      # (complex64: 64 x 64 with a second tile, 128 x 32 without)
    tri("two_tiles", _dt, _t, ("cba", "cab", "abc", "abc"), _two, ops=COMBINERS)
    tri("two_tiles_pad", _dt, _t, ("cba", "cab", "abc", "abc"), _two, n=2, pad={"A": 2, "B": 4, "C": 2, "D": 2})
    # two passes: tiled on both types; at an odd b the last pass of complex64 is the gather kernel
    _p2 = dict(passes=2, bothPermuted=0, variant_first=EW_TRANSPOSE, variant_inplace=EW_GENERIC)
    tri("two_pass", _dt, dict(a=68, b=34, c=12), ("cba", "bac", "abc", "abc"), dict(_p2, variant=EW_TRANSPOSE), ops=MM)
    tri("two_pass", _dt, dict(a=68, b=34, c=12), ("cba", "bac", "abc", "abc"), dict(_p2, variant=EW_TRANSPOSE), n=1)
    _odd = dict(_p2, variant=EW_GENERIC if _dt == "complex64" else EW_TRANSPOSE)
    tri("two_pass_odd", _dt, dict(a=68, b=33, c=12), ("cba", "bac", "abc", "abc"), _odd, n=2)
    # conjugation in every role
    for _k, _c in CONJ.items():
        tri("e_is_a_" + _k, _dt, _e, ("abc", "cab", "abc", "abc"), dict(_one, swapAB=0), conj3=_c, n=1)                    # A: E, B: tile operand
        tri("two_tiles_" + _k, _dt, _t, ("cba", "cab", "abc", "abc"), _two, conj3=_c, n=1)                                   # A: tile operand, B: X
        tri("rowcopy_" + _k, _dt, _r, ("abc", "acb", "abc", "abc"), _row, conj3=_c, n=1, cmodes=("separate",))
    tri("e_is_b_cABC", _dt, _e, ("cab", "abc", "abc", "abc"), dict(_one, swapAB=1), conj3=CONJ["cABC"], n=1)
    for _k in ("cA", "cB", "cABC"):                                                                                          # A: pass 1, B: the last pass
        tri("two_pass_" + _k, _dt, dict(a=68, b=34, c=12), ("cba", "bac", "abc", "abc"), dict(_p2, variant=EW_TRANSPOSE), conj3=CONJ[_k], n=1)

# the gather kernel on complex64: an element offset of 1 under descriptor alignment 8 leaves no 16-byte lanes
_g = dict(a=33, b=7, c=5)
_gen = dict(off=1, align=8)
_ge = dict(passes=1, bothPermuted=0, swapAB=0, variant=EW_GENERIC)
_g2 = dict(passes=2, bothPermuted=0, variant=EW_GENERIC, variant_first=EW_GENERIC, variant_inplace=EW_GENERIC)
tri("gather_e", "complex64", _g, ("abc", "cab", "abc", "abc"), _ge, ops=MM, **_gen)
tri("gather_e", "complex64", _g, ("abc", "cab", "abc", "abc"), _ge, n=1, **_gen)
tri("gather_two_pass", "complex64", _g, ("cba", "bac", "abc", "abc"), _g2, ops=MM, **_gen)
tri("gather_two_pass", "complex64", _g, ("cba", "bac", "abc", "abc"), _g2, n=1, **_gen)
for _k, _c in CONJ.items():
    tri("gather_e_" + _k, "complex64", _g, ("abc", "cab", "abc", "abc"), _ge, conj3=_c, n=1, **_gen)
tri("gather_two_pass_cABC", "complex64", _g, ("cba", "bac", "abc", "abc"), _g2, conj3=CONJ["cABC"], n=1, **_gen)              # (C is D: B is the gather kernel's X)

BY_ID = {c.id: c for c in CASES}
FORMS = {"e": lambda c: "_e_is_" in c.id, "rowcopy": lambda c: "_rowcopy" in c.id, "two_tiles": lambda c: "_two_tiles" in c.id,
         "two_pass": lambda c: "_two_pass" in c.id and "gather" not in c.id}


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def make_plan(ct, ops, h, case):
    m, e, s = case.modes, case.extents, case.strides
    cj = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in case.conj3]
    return ops.trinary_plan(h, e("A"), m["A"], e("B"), m["B"], e("C"), m["C"], e("D"), m["D"], opAB=case.op[0], opABC=case.op[1],
                            dtype=xc._dt(ct, case.dtype), alignment=case.align or 128, strideA=s("A"), strideB=s("B"), strideC=s("C"), strideD=s("D"),
                            opA=cj[0], opB=cj[1], opC=cj[2])


def plan_path(ct, ops, h, case):
    """the case's plan is on the path the case names (the planner needs no GPU), with complex scalars of the data's type; returns the description"""
    plan = make_plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d.raw)
        assert plan.scalar_type == xc._dt(ct, case.dtype), (case.id, plan.scalar_type)
        return {k: v for k, v in d.pairs}
    finally:
        plan.destroy()


# ---- reference ---------------------------------------------------------------------------------------------------------------------------
def assert_dyadic(x, what):
    """both parts of every value: magnitude below 2^14, a multiple of 1/8"""
    for part in (x.real, x.imag):
        assert float(np.abs(part).max()) < LIMIT, "%s: %g is not below 2^14" % (what, float(np.abs(part).max()))
        assert bool((part * GRAIN == np.round(part * GRAIN)).all()), "%s: not a multiple of 1/8" % what


def reference(case, ins, run, conj3=None, check=True):
    """the exact result of one run in complex128, D's modes in descriptor order; with `check` every intermediate is asserted exact in fp32"""
    scal, cmode = run
    cj = case.conj3 if conj3 is None else conj3
    m = case.modes

    def term(t, k):
        x = ins[t].astype(np.complex128)
        return complex(scal[k]) * ec.to_out(np.conj(x) if cj[k] else x, m[t], m["D"])
    a, b = term("A", 0), term("B", 1)
    out = ec.F[case.op[0]](a, b)
    steps = [("alpha A", a), ("beta B", b), ("opAB", out)]
    if cmode == "none":
        assert complex(scal[2]) == 0 and case.op[1] == "ADD", case.id
    else:
        c = term("C", 2)
        out = ec.F[case.op[1]](out, c)
        steps += [("gamma C", c), ("opABC", out)]
    if check:
        for name, x in steps:
            assert_dyadic(x, "%s %s" % (case.id, name))
    return np.broadcast_to(out, case.extents("D")).astype(np.complex128)


def check_data(case, ins):
    """both parts of every element an integer in [-3, 3]"""
    for t, x in ins.items():
        for part in (np.real(x), np.imag(x)):
            assert bool((part == np.round(part)).all()) and float(np.abs(part).max()) <= 3, (case.id, t)


def check_run(case, run):
    scal, _ = run
    for s in scal:
        assert abs(complex(s).real) in PARTS and abs(complex(s).imag) in PARTS, (case.id, s)
    assert any(complex(s).real != 0 and complex(s).imag != 0 for s in scal), (case.id, scal)


def check_case(case):
    """every draw and run of the case on the CPU: the data and scalar conditions, the reference's exactness and representability, and that
    a conjugation the case asks for shows in the result"""
    assert case.runs, case.id
    for draw in range(2):
        ins = ec.make_draw(case, draw, {})
        check_data(case, ins)
        for run in case.runs:
            check_run(case, run)
            ref = reference(case, ins, run)
            ec.expected(case, ref)
            if any(case.conj3) and not (run[1] == "none" and case.conj3 == (False, False, True)):
                plain = reference(case, ins, run, conj3=(False, False, False), check=False)
                assert bool((plain != ref).any()), "%s: the conjugation does not show" % case.id


# ---- running a case ----------------------------------------------------------------------------------------------------------------------
def run_case(ct, ops, h, case):
    import torch
    plan = make_plan(ct, ops, h, case)
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc), "%s is off its path: %s" % (case.id, desc.raw)
        for draw in range(2):
            ins = ec.make_draw(case, draw, {})
            dev = {}
            for t in "AB":
                dev[t] = ec._placed(case, t)
                dev[t].set(ec._host(case, ins[t]))
            for run in case.runs:
                scal, cmode = run
                check_run(case, run)
                want = ec.expected(case, reference(case, ins, run))
                pd = ec._placed(case, "D")                                     # NaN everywhere
                pc = None
                if cmode == "inplace":
                    pd.set(ec._host(case, ins["C"]))
                elif cmode == "separate":
                    pc = ec._placed(case, "C")
                    pc.set(ec._host(case, ins["C"]))
                plan.trinary(scal[0], dev["A"].ptr, scal[1], dev["B"].ptr, scal[2], pc.ptr if pc else pd.ptr, pd.ptr)
                torch.cuda.synchronize()
                what = "%s (draw %d, scalars %s, C %s) %s" % (case.id, draw, scal, cmode, desc.raw)
                xd.assert_exact(pd.get(), want, what)
                pd.check_outside(what)
                for t in "AB":
                    xd.assert_exact(dev[t].get(), ec._host(case, ins[t]), what + ": %s was written" % t)
                    dev[t].check_outside(what + " (%s)" % t)
                if pc is not None:
                    xd.assert_exact(pc.get(), ec._host(case, ins["C"]), what + ": C was written")
                    pc.check_outside(what + " (C)")
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
