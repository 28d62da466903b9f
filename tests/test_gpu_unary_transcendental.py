"""EXP, LOG, TANH and SIGMOID as the unary operator of a permutation's operand (alpha = 1), on one transposing, one row-copy and one
element-gather geometry per real data type (the geometries and guarded buffers of tests/ew_exact_cases.py), and sum exp(a) on every fp32
reduction variant with and without a split.

Inputs: a dense grid over [-10, 10] (LOG: over [2^-10, 2^10], geometric; TANH: over [-5, 5]), one grid point per element, shuffled, rounded
to the data type.  Reference: numpy in fp64 on the rounded inputs.

Bounds.  fp32 / fp64 data: measured here against the device's own library — torch evaluates the same function on the same GPU tensor, its
maximal error in ulps of the arithmetic type against the fp64 reference is T; the engine's maximal error must not exceed T + 1 ulp (two
correct evaluations of one function may differ in the last rounding).  bf16 / fp16 data: the result is the fp64 reference rounded to the
type, or one of its two neighbours in the type (an fp32 evaluation a few ulp32 off moves the 16-bit rounding by at most one step).
Reductions: |got - ref| <= (u + red * 2^-24) * |alpha| * sum |exp a| with u = (T + 1) * 2^-23, the relative per-element bound just measured,
and red * 2^-24 for the fp32 additions.  Each test prints its figures before it asserts (pytest -s shows them)."""
import numpy as np
import pytest

import ew_exact_cases as ec
import exact_data as xd
import unary_cases as uc
import workspace_cases as wc

pytestmark = pytest.mark.gpu

OPS = ("EXP", "LOG", "TANH", "SIGMOID")
FN = {"EXP": np.exp, "LOG": np.log, "TANH": np.tanh, "SIGMOID": lambda x: 1.0 / (1.0 + np.exp(-x))}
_F16_GENERIC = ec.Case("f16_perm_generic", "permutation", "float16", dict(a=33, b=170, c=7), ("abc", "acb"), ec._is(variant=ec.EW_GENERIC),
                       [((1.0,), "none")], pad={"A": 1, "D": 2}, off=3, align=2)
GEOMETRIES = {          # data type -> (transposing, row copy, element gather)
    "float32": ("f32_perm_transpose_t64_pad", "f32_perm_rowcopy_pad", "f32_perm_generic"),
    "float64": ("f64_perm_transpose_pad", "f64_perm_rowcopy_pad", "f64_perm_generic"),
    "bfloat16": ("bf16_perm_transpose_w256", "bf16_perm_rowcopy_pad", "bf16_perm_generic"),
    "float16": ("f16_perm_transpose_w256", "f16_perm_rowcopy_pad", "f16_perm_generic"),
}
REDUCTIONS = ("f32_red_col_add", "f32_red_col_split_add", "f32_red_row_add", "f32_red_row_split_add", "f32_red_gen_digits_add", "f32_red_gen_split_add",
              "f32_red_rowany_add", "f32_red_rowany_split_add")


def _base(bid):
    return _F16_GENERIC if bid == "f16_perm_generic" else ec.BY_ID[bid]


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def grid(op, n, dtype, seed):
    """n grid points of the operator's interval, shuffled, rounded to the data type (float64 values of the type)"""
    import torch
    if op == "LOG":
        x = 2.0 ** np.linspace(-10.0, 10.0, n)
    else:
        lim = 5.0 if op == "TANH" else 10.0
        x = np.linspace(-lim, lim, n)
    np.random.default_rng(seed).shuffle(x)
    return torch.from_numpy(x).to(xd.TORCH_DTYPES[dtype]).to(torch.float64).numpy()


def ulps(got, ref, dtype):
    """max |got - ref| in ulps of the arithmetic type (fp32 / fp64) at |ref|"""
    ref = np.asarray(ref, dtype=np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) if dtype == "float32" else np.spacing(np.abs(ref))
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / ulp).max())


def ordinal16(t):
    """a 16-bit floating-point tensor's values as integers that count the type's values in order"""
    import torch
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


_TORCH = {}


def torch_ulps(op, dtype, x_dev, ref):
    """T: the device library's own maximal error on this tensor, through torch"""
    import torch
    fn = {"EXP": torch.exp, "LOG": torch.log, "TANH": torch.tanh, "SIGMOID": torch.sigmoid}[op]
    t = ulps(fn(x_dev).cpu().numpy(), ref, dtype)
    _TORCH[(op, dtype)] = max(t, _TORCH.get((op, dtype), 0.0))
    return t


@pytest.mark.parametrize("which", (0, 1, 2), ids=("transpose", "rowcopy", "generic"))
@pytest.mark.parametrize("dtype", sorted(GEOMETRIES))
def test_transcendental_permutation(env, dtype, which):
    import torch
    ct, ops, h = env
    base = _base(GEOMETRIES[dtype][which])
    n = int(np.prod(base.extents("A")))
    pa, pd = ec._placed(base, "A"), ec._placed(base, "D")
    for op in OPS:
        case = uc.UCase(base, dict(A=op), op.lower())
        plan = uc.make_plan(ct, ops, h, base, case.un)
        try:
            desc = wc.describe(ct, plan)
            assert base.expect(desc) and desc.get("unary") == [ops._UNARY[op], ct.OP_IDENTITY, ct.OP_IDENTITY], desc.pairs
            x = grid(op, n, dtype, which).reshape(base.extents("A"))                       # modes in descriptor order
            ref = ec.reference(base, {"A": FN[op](x)}, ((1.0,), "none"))
            pa.set(ec._host(base, x))
            pd.refill_nan()
            plan.permute(1.0, pa.ptr, pd.ptr)
            torch.cuda.synchronize()
            got = pd.get()
            what = "%s %s %s" % (base.id, op, desc.pairs)
            pd.check_outside(what)
            if dtype in xd.H16:
                want = torch.from_numpy(np.ascontiguousarray(ref)).to(torch.float32).to(xd.TORCH_DTYPES[dtype])
                steps = int((ordinal16(got) - ordinal16(want)).abs().max())
                print("UNARY16 %s %s %s: %d step(s) of the type from the rounded reference" % (dtype, op, base.id, steps))
                assert not bool(torch.isnan(got.float()).any()), what
                assert steps <= 1, what
            else:
                x_dev = ec._host(base, x).cuda()
                t = torch_ulps(op, dtype, x_dev, FN[op](x))
                e = ulps(got.numpy(), ref, dtype)
                print("UNARYULP %s %s %s: torch %.3f ulp, engine %.3f ulp" % (dtype, op, base.id, t, e))
                assert e <= t + 1.0, what
        finally:
            plan.destroy()


@pytest.mark.parametrize("bid", REDUCTIONS)
def test_sum_of_exp(env, bid):
    import torch
    ct, ops, h = env
    base = ec.BY_ID[bid]
    case = uc.UCase(base, dict(A="EXP"), "exp")
    d = uc.plan_path(ct, ops, h, case)
    kept, red, _ = ec._lines(base)
    x = ec._from_lines(base, grid("EXP", kept * red, "float32", 7).reshape(kept, red))
    # u: the per-element bound, from the device library's error on this very tensor
    t = torch_ulps("EXP", "float32", ec._host(base, x).cuda(), np.exp(x))
    u = (t + 1.0) * 2.0 ** -23
    alpha = -0.5
    run = ((alpha, 0.0), "none")
    ref = ec.reference(base, {"A": np.exp(x), "C": np.zeros(base.extents("D"))}, run)
    mag = ec.reference(base, {"A": np.exp(x), "C": np.zeros(base.extents("D"))}, ((abs(alpha), 0.0), "none"))       # |alpha| sum |exp a|
    plan = uc.make_plan(ct, ops, h, base, case.un)
    try:
        pa, pd = ec._placed(base, "A"), ec._placed(base, "D")
        pa.set(ec._host(base, x))
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        plan.reduce(alpha, pa.ptr, 0.0, pd.ptr, pd.ptr, ws.data_ptr(), plan.required_workspace)
        torch.cuda.synchronize()
        got = pd.get().to(torch.float64).numpy()
        pd.check_outside(bid)
        err = np.abs(got - ref) / mag
        bound = u + red * 2.0 ** -24
        print("UNARYSUM %s: variant %d rowAny %d splitR %d red %d: torch exp %.3f ulp, relative error %.3g of bound %.3g" %
              (bid, d["variant"], d["rowAny"], d["splitR"], red, t, float(err.max()), bound))
        assert bool((err <= bound).all()), (bid, float(err.max()), bound)
    finally:
        plan.destroy()
