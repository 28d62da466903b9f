"""The one branch of cutensorElementwiseTrinaryExecute no other test reaches: a two-pass plan WITHOUT a single-launch form, called in
place.  Pass 1 would overwrite C before the last pass reads it, and the element-gather launch that replaces both passes cannot describe
the problem — the call is refused (CUTENSOR_STATUS_NOT_SUPPORTED) before anything runs.

D = C = "abcdefg" packed, A = "gfedcab", B = "baedcfg", every extent 2 except a = g = 3 (288 elements): pass 1 (A -> D) fuses ab, the last
pass (B, C -> D) fuses fg — six groups each, four rest modes —, the joint plan of A, B, C and D fuses nothing: seven groups, five rest
modes, one more than the kernels' argument block holds.  The description says so on the CPU (passes 2, variant_inplace -1).

On the GPU, in guarded NaN-filled buffers, integer data, no tolerance: C apart from D is exact; C = D with gamma = 0 under ADD reads no C,
runs the two passes and is exact; C = D with gamma = 2 is refused, D bit for bit what it was, every guard intact."""
import numpy as np
import pytest
import torch

import exact_data as xd
import guarded as gd

EXT = dict(a=3, b=2, c=2, d=2, e=2, f=2, g=3)
MODES = dict(A="gfedcab", B="baedcfg", C="abcdefg", D="abcdefg")
DTYPES = ("float32", "complex64")
ALPHA_BETA = {"float32": (2.0, -1.0), "complex64": (1 + 2j, -1 + 1j)}
GAMMA = 2.0


def extents(t):
    return [EXT[c] for c in MODES[t]]


def make_plan(ct, ops, h, dtype):
    dt = {"float32": ct.R_32F, "complex64": ct.C_32F}[dtype]
    return ops.trinary_plan(h, extents("A"), MODES["A"], extents("B"), MODES["B"], extents("C"), MODES["C"], extents("D"), MODES["D"],
                            opAB="ADD", opABC="ADD", dtype=dt)


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_plan_has_two_passes_and_no_single_launch_form(env, dtype):
    ct, ops, h = env
    plan = make_plan(ct, ops, h, dtype)
    try:
        d = plan.describe()
        assert d["form"] == "trinary" and d["passes"] == 2 and d["variant_inplace"] == -1, d
    finally:
        plan.destroy()


def _data(dtype):
    """logical host tensors of integers in [-3, 3] (complex: both parts), modes in descriptor order"""
    out = {}
    for i, t in enumerate("ABC"):
        rng = np.random.default_rng([20240517, i])
        parts = [xd._dense(rng, extents(t), range(-3, 4)) for _ in range(2 if dtype == "complex64" else 1)]
        out[t] = xd._to_torch(tuple(parts) if dtype == "complex64" else parts[0], dtype)
    return out


def _want(dtype, ins, gamma):
    w = gd.wide(dtype)
    to_d = lambda t: ins[t].to(w).permute([MODES[t].index(c) for c in MODES["D"]])   # noqa: E731
    alpha, beta = ALPHA_BETA[dtype]
    ref = alpha * to_d("A") + beta * to_d("B") + (gamma * to_d("C") if gamma else 0.0)
    want = xd.round_to(ref, dtype)
    assert bool((want == ref).all())                      # every exact output is a value of the data type: nothing rounds
    return want


@pytest.fixture(scope="module", params=DTYPES)
def case(request, env):
    ct, ops, h = env
    dtype = request.param
    ins = _data(dtype)
    dev = {}
    for t in "AB":
        dev[t] = gd.guarded_tensor(extents(t), dtype)
        dev[t].set(ins[t])
    plan = make_plan(ct, ops, h, dtype)
    yield ct, plan, dtype, ins, dev, {g: _want(dtype, ins, g) for g in (GAMMA, 0.0)}
    plan.destroy()


def _run(plan, dtype, dev, gamma, c, d):
    alpha, beta = ALPHA_BETA[dtype]
    plan.trinary(alpha, dev["A"].ptr, beta, dev["B"].ptr, gamma, c.ptr, d.ptr)
    torch.cuda.synchronize()


def _check_inputs(ins, dev, what):
    for t in "AB":
        xd.assert_exact(dev[t].get(), ins[t], what + ": %s was written" % t)
        dev[t].check_guard(what + " (%s)" % t)


@pytest.mark.gpu
def test_c_apart_from_d_is_exact(case):
    ct, plan, dtype, ins, dev, want = case
    c, d = gd.guarded_tensor(extents("C"), dtype), gd.guarded_tensor(extents("D"), dtype)
    c.set(ins["C"])
    _run(plan, dtype, dev, GAMMA, c, d)
    what = "%s, C apart from D" % dtype
    xd.assert_exact(d.get(), want[GAMMA], what)
    d.check_guard(what)
    xd.assert_exact(c.get(), ins["C"], what + ": C was written")
    c.check_guard(what + " (C)")
    _check_inputs(ins, dev, what)


@pytest.mark.gpu
def test_in_place_with_gamma_zero_runs_and_is_exact(case):
    ct, plan, dtype, ins, dev, want = case
    d = gd.guarded_tensor(extents("D"), dtype)             # NaN everywhere: a C term that was read would show
    _run(plan, dtype, dev, 0.0, d, d)
    what = "%s, C is D, gamma = 0" % dtype
    xd.assert_exact(d.get(), want[0.0], what)
    d.check_guard(what)
    _check_inputs(ins, dev, what)


@pytest.mark.gpu
def test_in_place_with_gamma_two_is_refused_before_anything_runs(case):
    ct, plan, dtype, ins, dev, want = case
    d = gd.guarded_tensor(extents("D"), dtype)
    d.set(ins["C"])
    before = d.bits()
    with pytest.raises(ct.CuTensorError) as e:
        _run(plan, dtype, dev, GAMMA, d, d)
    assert e.value.status == ct.STATUS_NOT_SUPPORTED, e.value
    torch.cuda.synchronize()
    what = "%s, C is D, gamma = 2" % dtype
    assert np.array_equal(d.bits(), before), what + ": D or its guards changed"
    d.check_guard(what)
    _check_inputs(ins, dev, what)
