"""cutensorElementwiseTrinaryExecute on complex data with ordinary values: N(0, 1) parts in every input and scalar, one shape per form and
per type (the shapes of tests/cplx_trinary_cases.py), against numpy in complex128 — and the two-pass form's stream order.

The bound per component is 16 u mag, u = 2^-24 (complex64) / 2^-53 (complex128), mag = the expression evaluated on |re| + |im| of every
input and scalar (a component of a complex product is at most the product of its factors' |re| + |im|).  Derived, not measured: at most
three complex products and two sums lie on any path from an input to the output (the scaling, opAB as MUL, opABC as MUL; the two
combiners as sums), each costs at most 3 roundings per component (two real products and their sum), so the relative error of the
magnitude-weighted result stays below (1 + u)^9 - 1 < 10 u; the two-pass form stores alpha * cj(A) in the data's own type, the precision it
was computed in, which adds nothing.  16 leaves room for the reference's own rounding in complex128 on the complex64 cases and nothing
else.

The stream-order case: both launches of the two-pass form go on the caller's stream while that stream is still blocked and its inputs
hold NaN (tests/stream_cases.py)."""
import numpy as np
import pytest

import cplx_trinary_cases as tc
import ew_exact_cases as ec
import stream_cases as sc
import workspace_cases as wc

pytestmark = pytest.mark.gpu

U = {"complex64": 2.0 ** -24, "complex128": 2.0 ** -53}
# form -> (extents, modes A B C D, a predicate's fields, padded pitches, (offset, alignment))
E_, R_, T_, P_, G_ = dict(a=130, b=3, c=66), dict(a=256, b=12, c=10), dict(a=130, b=4, c=66), dict(a=68, b=34, c=12), dict(a=33, b=7, c=5)
FORMS = {
    "e_is_a": (E_, ("abc", "cab", "cba", "abc"), dict(passes=1, bothPermuted=0, swapAB=0, variant=tc.EW_TRANSPOSE), {}, (0, None)),
    "e_is_b": (E_, ("cab", "abc", "abc", "abc"), dict(passes=1, bothPermuted=0, swapAB=1, variant=tc.EW_TRANSPOSE), {}, (0, None)),
    "rowcopy": (R_, ("abc", "acb", "abc", "abc"), dict(passes=1, variant=tc.EW_ROWCOPY), {"A": 2, "B": 4, "C": 2, "D": 2}, (0, None)),
    "two_tiles": (T_, ("cba", "cab", "abc", "abc"), dict(passes=1, bothPermuted=1, variant=tc.EW_TRANSPOSE), {"A": 2, "B": 4, "C": 2, "D": 2}, (0, None)),
    "two_pass": (P_, ("cba", "bac", "abc", "abc"), dict(passes=2, variant=tc.EW_TRANSPOSE, variant_first=tc.EW_TRANSPOSE), {}, (0, None)),
    "two_pass_inplace": (P_, ("cba", "bac", "abc", "abc"), dict(passes=2, variant_inplace=tc.EW_GENERIC), {}, (0, None)),
    "gather": (G_, ("abc", "cab", "abc", "abc"), dict(passes=1, variant=tc.EW_GENERIC), {}, (1, 8)),
}
PARAMS = [(dt, f) for dt in tc.DTYPES for f in FORMS if not (f == "gather" and dt == "complex128")]


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def _normal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("dtype,form", PARAMS, ids=["%s_%s" % (ec.SHORT[d], f) for d, f in PARAMS])
def test_parity_with_numpy(env, dtype, form):
    import torch
    ct, ops, h = env
    ext, modes, want, pad, (off, align) = FORMS[form]
    k = sorted(FORMS).index(form)
    op = tc.COMBINERS[(k + (dtype == "complex128")) % 4] if form != "two_tiles" else ("MUL", "MUL")
    conj3 = tuple(bool((k >> i) & 1) for i in range(3))
    case = tc.Case("parity_%s_%s" % (ec.SHORT[dtype], form), dtype, ext, modes, tc._want(conj3, **want), [], op, conj3, pad=pad, off=off, align=align)
    rng = np.random.default_rng([2024, k, tc.DTYPES.index(dtype)])
    scal = [complex(_normal(rng, ())) for _ in range(3)]
    ins = {t: _normal(rng, case.extents(t)) for t in "ABC"}
    host = {t: ec._host(case, x) for t, x in ins.items()}                         # rounded to the data's type: what the kernel is given
    given = {t: host[t].to(torch.complex128).numpy() for t in "ABC"}

    def evaluate(x, s, cj):
        term = lambda t, i: s[i] * ec.to_out(np.conj(x[t]) if cj[i] else x[t], case.modes[t], case.modes["D"])   # noqa: E731
        return ec.F[op[1]](ec.F[op[0]](term("A", 0), term("B", 1)), term("C", 2))
    m1 = lambda z: np.abs(np.real(z)) + np.abs(np.imag(z))   # noqa: E731
    if dtype == "complex64":                                                       # the scalars as the library receives them
        scal = [complex(np.complex64(s)) for s in scal]
    ref = evaluate(given, scal, conj3)
    mag = evaluate({t: m1(x) for t, x in given.items()}, [m1(s) for s in scal], (False, False, False)).real
    plan = tc.make_plan(ct, ops, h, case)
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc), "%s is off its path: %s" % (case.id, desc.raw)
        dev = {t: ec._placed(case, t) for t in "ABD"}
        for t in "AB":
            dev[t].set(host[t])
        inplace = form == "two_pass_inplace"
        pc = dev["D"] if inplace else ec._placed(case, "C")
        pc.set(host["C"])
        plan.trinary(scal[0], dev["A"].ptr, scal[1], dev["B"].ptr, scal[2], pc.ptr, dev["D"].ptr)
        torch.cuda.synchronize()
        got = dev["D"].get().to(torch.complex128).numpy()
        dev["D"].check_outside(case.id)
    finally:
        plan.destroy()
    err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
    worst = float((err / mag).max()) / U[dtype]
    print("PARITY %s %s %s: worst component error %.2f u mag (bound 16)" % (case.id, op, conj3, worst), flush=True)
    assert bool(np.isfinite(got.real).all() and np.isfinite(got.imag).all()), case.id
    assert worst <= 16.0, "%s: %.2f u mag %s" % (case.id, worst, desc.raw)


def test_both_passes_of_the_two_pass_form_follow_the_caller_s_stream(env):
    ct, ops, h = env
    case = tc.BY_ID["c64_tri_two_pass_mul_mul"]
    run = next(r for r in case.runs if r[1] == "separate")
    plan = tc.make_plan(ct, ops, h, case)
    desc = wc.describe(ct, plan)
    assert case.expect(desc) and desc.get("passes") == 2, desc.raw
    dev = {t: ec._placed(case, t) for t in "ABC"}
    pd = ec._placed(case, "D")
    ins = [dev[t] for t in "ABC"]
    draws = []
    for draw in range(2):
        x = ec.make_draw(case, draw, {})
        want = ec.expected(case, tc.reference(case, x, run))
        draws.append((sc.stage(ins, [ec._host(case, x[t]) for t in "ABC"]), [want]))
    scal = run[0]

    def launch(stream):
        plan.trinary(scal[0], dev["A"].ptr, scal[1], dev["B"].ptr, scal[2], dev["C"].ptr, pd.ptr, stream)
    p = sc.Prepared("%s scalars %s C separate %s" % (case.id, scal, desc.raw), plan, ins, [pd], None, launch, draws)
    try:
        for k in (0, 1):
            sc.gated([(p, k, sc.side_stream(0))])
    finally:
        p.close()
