"""The ONE rounding of a converting permutation, D = rnd_D(alpha * uA(cmp(perm A))) — the integer data of tests/test_gpu_convert_exact.py
never rounds.  Each narrowing pair (fp32 -> bf16, fp32 -> fp16, fp64 -> fp32) runs on each of the three forms (the row-copy, transposing
and element-gather shapes of tests/convert_cases.py) with A filled by cycling through a fixed vector of A's type, built from the target
type's parameters (p = its precision in bits, eps = 2^(1-p), tiny = its smallest normal number, sub = tiny * eps its smallest subnormal, u
= A's own spacing at 1):

  * ties: 1 + eps/2 (between 1 and 1 + eps: to even = down) and 1 + 3 eps/2 (to even = up) — for fp32 -> bf16 1 + 2^-8 and 1 + 3 * 2^-8;
    each tie +- u, just above and just below; all of it with both signs;
  * the largest finite value M, M + half its spacing (the first value that rounds to inf) and one u-step below that (rounds to M);
  * the subnormal range: 0.75 tiny (a subnormal of the type), 2.5 sub and 3.5 sub (ties to 2 sub and 4 sub), 2.5 sub (1 + 2^-10) (to 3 sub),
    0.75 sub (to sub), sub / 2 (a tie: to zero), sub / 2 (1 + 2^-10) (to sub), sub / 4 (to zero), with both signs (a negative one gives -0);
  * +-0, +-inf, NaN, and a few ordinary values.

alpha is 1 and 0.5 (exact in the compute type).  alpha * a stays a normal number of the compute type for fp32 -> fp16 and fp64 -> fp32;
for fp32 -> bf16 it cannot — the subnormals of bf16 ARE the subnormals of fp32, the compute type — so those entries also hold the
library to IEEE arithmetic on fp32 subnormals, as the reference's.  The comparison is bit for bit against torch on the CPU,
(alpha * a.to(cmp)).to(D), NaN where it has NaN.  The widening pairs run on the same vector rounded to A's type and must be exact,
subnormals included.

Unary operators: per pair, on the transposing shape, RELU / ABS / NEG on signed and SQRT / RCP on positive non-integer data.  SQRT and RCP
are correctly rounded (unary_op.h), so the correctly rounded operation on the CPU in the compute type, then torch's .to(D), is bit for bit
the answer.  For RELU / ABS / NEG / RCP that is torch's own.  torch.sqrt on the CPU is NOT correctly rounded (its vectorised kernels miss
the last bit of fp32 and of fp64 on a share of ordinary values that depends on the host's instruction set — from under 1 % to over 20 % —
as 50-digit arithmetic shows; the library's results were the nearer ones), so the SQRT reference is numpy's sqrt in the compute type, the
IEEE instruction, and correctly_rounded_sqrt proves it before it is used: in fp32 against the sqrt taken in fp64 and rounded (53 >= 2 * 24 + 2
bits: the second rounding cannot change the result), in fp64 against 50-digit arithmetic on a sample.  EXP (fp32 -> bf16): the
bound tests/test_gpu_unary_transcendental.py allows the operator in fp32 — T + 1 ulp of fp32 at the fp64 reference, T the device library's own
maximal error on this tensor, through torch — plus half an ulp of bf16 for the final rounding."""
import numpy as np
import pytest

import convert_cases as cc
import exact_data as xd
import workspace_cases as wc

pytestmark = pytest.mark.gpu

NARROWING = (("float32", "bfloat16"), ("float32", "float16"), ("float64", "float32"))
WIDENING = tuple((d, a) for a, d in NARROWING)
PRECISION = {"bfloat16": (8, 127, -126), "float16": (11, 15, -14), "float32": (24, 127, -126)}        # p, emax, emin
FORMS = ("rowcopy", "transpose", "generic")
ALPHAS = (1.0, 0.5)


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def vector(pair):
    """the fixed vector of a narrowing pair as a tensor of A's type; every entry is asserted to be a value of A's type"""
    import torch
    a, d = pair
    p, emax, emin = PRECISION[d]
    eps, tiny = 2.0 ** (1 - p), 2.0 ** emin
    sub = tiny * eps
    u = 2.0 ** -23 if a == "float32" else 2.0 ** -52
    top = (2.0 - eps / 2) * 2.0 ** emax                        # M + half its spacing: a tie between M (odd) and 2^(emax + 1) = inf
    pos = [1 + eps / 2, 1 + 3 * eps / 2, 1 + eps / 2 + u, 1 + eps / 2 - u, 1 + 3 * eps / 2 + u, 1 + 3 * eps / 2 - u,
           (2.0 - eps) * 2.0 ** emax, top, top - u * 2.0 ** emax,
           0.75 * tiny, 2.5 * sub, 3.5 * sub, 2.5 * sub * (1 + 2.0 ** -10), 0.75 * sub, sub / 2, sub / 2 * (1 + 2.0 ** -10), sub / 4,
           1.0, 2.5, 3.14159, 1.0 / 3.0]
    vals = np.asarray(pos + [-x for x in pos] + [0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float64)
    t = torch.from_numpy(vals).to(xd.TORCH_DTYPES[a])
    back = t.to(torch.float64).numpy()
    exact = (back == vals) | np.isnan(vals)
    if a == "float32":
        exact[[pos.index(3.14159), pos.index(1.0 / 3.0)]] = True          # (the ordinary values are whatever fp32 makes of them)
        exact[[len(pos) + pos.index(3.14159), len(pos) + pos.index(1.0 / 3.0)]] = True
    assert bool(exact.all()), (pair, vals[~exact])
    return t


def bits(t):
    import torch
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same_bits(got, want, what):
    import torch
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert bool((torch.isnan(got) == nan).all()), "%s: NaN positions differ" % what
    bad = (bits(got) != bits(want)) & ~nan
    n = int(bad.sum())
    if n:
        at = torch.nonzero(bad)[:6]
        lines = ["  %s: got %r (%#x), expected %r (%#x)" % (tuple(int(i) for i in ix), got[tuple(ix)].item(), int(bits(got)[tuple(ix)]) & (2 ** (8 * got.element_size()) - 1),
                                                            want[tuple(ix)].item(), int(bits(want)[tuple(ix)]) & (2 ** (8 * got.element_size()) - 1)) for ix in at]
        raise AssertionError("%s: %d of %d elements differ in their bits; the first:\n%s" % (what, n, got.numel(), "\n".join(lines)))


def cmp_type(pair):
    import torch
    return torch.float64 if "float64" in pair else torch.float32


def cycled(vec, case):
    """A (modes in descriptor order) filled by cycling through vec"""
    import torch
    ext = case.extents("A")
    n = int(np.prod(ext))
    return vec[torch.arange(n) % vec.numel()].reshape(ext)


def to_d_order(case, x):
    mA, mD = case.modes["A"], case.modes["D"]
    return x.permute([mA.index(c) for c in mD]).contiguous()


def run_permutation(env, case, a_host, alpha, un=None, predicate=None):
    """one launch of the case's converting permutation on a_host (A's type, descriptor order); returns D as a CPU tensor of D's type"""
    import torch
    ct, ops, h = env
    plan = cc.make_plan(ct, ops, h, case, un=un)
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc) and (predicate is None or predicate(desc)), "%s is off its path: %s" % (case.id, desc.raw)
        pa, pd = cc.placed(case, "A"), cc.placed(case, "D")
        pa.set(a_host)
        plan.permute(alpha, pa.ptr, pd.ptr)
        torch.cuda.synchronize()
        pd.check_outside("%s %s" % (case.id, desc.raw))
        return pd.get(), desc.raw
    finally:
        plan.destroy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pair", NARROWING + WIDENING, ids=[cc._name(p) for p in NARROWING + WIDENING])
def test_one_rounding_to_nearest_even(env, pair, form):
    import torch
    case = cc.BY_ID["%s_perm_%s" % (cc._name(pair), form)]
    narrowing = pair in NARROWING
    vec = vector(pair) if narrowing else vector((pair[1], pair[0])).to(xd.TORCH_DTYPES[pair[0]])     # widening: the vector rounded to A's type
    a = cycled(vec, case)
    for alpha in ALPHAS:
        want = to_d_order(case, (a.to(cmp_type(pair)) * alpha).to(xd.TORCH_DTYPES[pair[1]]))
        if not narrowing:            # widening never rounds: the reference itself is exact
            assert bool(((want.to(torch.float64) == a.to(torch.float64).permute([case.modes["A"].index(c) for c in case.modes["D"]]) * alpha) | torch.isnan(want)).all())
        got, raw = run_permutation(env, case, a, alpha)
        assert_same_bits(got, want, "%s alpha %s %s" % (case.id, alpha, raw))


def test_the_vectors_round_as_the_docstring_says():
    """on the CPU reference alone: ties go to even on both sides, M + half a spacing is inf, the subnormal entries land where they should"""
    import torch
    for pair in NARROWING:
        p, emax, emin = PRECISION[pair[1]]
        eps, tiny = 2.0 ** (1 - p), 2.0 ** emin
        sub = tiny * eps
        r = vector(pair).to(xd.TORCH_DTYPES[pair[1]]).to(torch.float64).numpy()
        assert list(r[:6]) == [1.0, 1 + 2 * eps, 1 + eps, 1.0, 1 + 2 * eps, 1 + eps], (pair, r[:6])
        M = (2.0 - eps) * 2.0 ** emax
        assert list(r[6:9]) == [M, np.inf, M], (pair, r[6:9])
        assert list(r[9:17]) == [0.75 * tiny, 2 * sub, 4 * sub, 3 * sub, sub, 0.0, sub, 0.0], (pair, r[9:17])


def correctly_rounded_sqrt(x):
    """the correctly rounded square root of a CPU tensor of the compute type, in that type (see the docstring: torch.sqrt is not that)"""
    import torch
    from decimal import Decimal, getcontext
    v = x.contiguous().numpy()
    r = np.sqrt(v)
    assert r.dtype == v.dtype
    if v.dtype == np.float32:
        assert bool((r == np.sqrt(v.astype(np.float64)).astype(np.float32)).all()), "numpy's fp32 sqrt is not the rounded fp64 one"
    else:
        getcontext().prec = 50
        for xi, ri in zip(v.reshape(-1)[:512].tolist(), r.reshape(-1)[:512].tolist()):
            exact = Decimal(xi).sqrt()
            err = abs(Decimal(ri) - exact)
            assert all(err <= abs(Decimal(float(c)) - exact) for c in (np.nextafter(ri, 0.0), np.nextafter(ri, np.inf))), (xi, ri)
    return torch.from_numpy(r)


UNARY = {"RELU": lambda x: x.relu(), "ABS": lambda x: x.abs(), "NEG": lambda x: -x, "SQRT": correctly_rounded_sqrt, "RCP": lambda x: 1.0 / x}


@pytest.mark.parametrize("pair", cc.PAIRS, ids=[cc._name(p) for p in cc.PAIRS])
def test_exact_unary_operators_in_the_compute_type(env, pair):
    import torch
    ct, ops, _ = env
    case = cc.BY_ID["%s_perm_transpose" % cc._name(pair)]
    n = int(np.prod(case.extents("A")))
    rng = np.random.default_rng(20 + cc.PAIRS.index(pair))
    for i, (op, fn) in enumerate(UNARY.items()):
        x = rng.uniform(0.25, 4.0, n)
        if op in ("RELU", "ABS", "NEG"):
            x = x * rng.choice([-1.0, 1.0], n)
        a = torch.from_numpy(x).to(xd.TORCH_DTYPES[pair[0]]).reshape(case.extents("A"))
        assert not bool((a.to(torch.float64) == a.to(torch.float64).round()).all())
        alpha = ALPHAS[i % 2]
        want = to_d_order(case, (fn(a.to(cmp_type(pair))) * alpha).to(xd.TORCH_DTYPES[pair[1]]))
        got, raw = run_permutation(env, case, a, alpha, un={"A": op},
                                   predicate=lambda d: d.get("unary") == [ops._UNARY[op], ct.OP_IDENTITY, ct.OP_IDENTITY])
        assert_same_bits(got, want, "%s %s alpha %s %s" % (case.id, op, alpha, raw))


def test_exp_in_fp32_then_one_rounding_to_bf16(env):
    import torch
    ct, ops, _ = env
    pair = ("float32", "bfloat16")
    case = cc.BY_ID["%s_perm_transpose" % cc._name(pair)]
    n = int(np.prod(case.extents("A")))
    x = np.linspace(-10.0, 10.0, n)
    np.random.default_rng(5).shuffle(x)
    a = torch.from_numpy(x).to(torch.float32).reshape(case.extents("A"))
    x = a.to(torch.float64).numpy()
    ref = np.exp(x)
    spacing32 = np.spacing(ref.astype(np.float32)).astype(np.float64)
    t = float((np.abs(torch.exp(a.cuda()).cpu().to(torch.float64).numpy() - ref) / spacing32).max())        # T: the device library's own error
    ulp_bf16 = 2.0 ** (np.floor(np.log2(ref)) - 7)
    bound = (t + 1.0) * spacing32 + 0.5 * ulp_bf16
    got, raw = run_permutation(env, case, a, 1.0, un={"A": "EXP"}, predicate=lambda d: d.get("unary") == [ct.OP_EXP, ct.OP_IDENTITY, ct.OP_IDENTITY])
    err = np.abs(got.to(torch.float64).numpy() - to_d_order(case, torch.from_numpy(ref)).numpy())
    worst = float((err / to_d_order(case, torch.from_numpy(bound)).numpy()).max())
    print("CONVERTEXP torch exp %.3f ulp32; worst error %.3f of the bound (T + 1 ulp32 + 0.5 ulp of bf16)" % (t, worst))
    assert worst <= 1.0, raw
