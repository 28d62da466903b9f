"""The mixed fp64 x complex128 contraction (csrc/kernels/gett_gen_rc64.inc and its routes) on the GPU, bit for bit: every case of
tests/rc64_cases.py on integer-valued data in NaN-guarded buffers against the CPU's complex128 result with the real operand widened, the
einsum front end on the same data, and one random-data case per layout against a bound from the fp64 accumulation.

Every test here fails on a library without the feature at cutensorCreateContraction (NOT_SUPPORTED: "mixed data types")."""
import pytest
import torch

import exact_cases as xc
import exact_data as xd
import rc64_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", rc.IN_PROCESS)
def test_case_is_exact(env, cid):
    ct, ops, h = env
    rc.run_case(ct, ops, h, rc.BY_ID[cid])


def test_conj_on_the_real_operand_equals_identity(env):
    """the same problem and data with and without CONJ on the real operand: the same bits"""
    ct, ops, h = env
    for real in (0, 1):
        c = rc.BY_ID["conj_on_real_%s" % "AB"[real]]
        plain = rc.Case(c.id, c.ext, c.modes, c.real, c.expect, beta=c.beta)       # (the same id: the same draws)
        assert torch.equal(rc.reference(c, *rc.make_inputs(c, False)), rc.reference(plain, *rc.make_inputs(plain, False)))
        rc.run_case(ct, ops, h, plain)


@pytest.mark.parametrize("group", rc.GROUPS)
def test_cases_behind_a_process_wide_switch(group):
    """CUTENSOR_AMD_PEEL=0: the wide view reaches the mode-table kernel, which reads the real operand as reals"""
    cases = [c for c in rc.CASES if c.group == group]
    xc.in_child([c.id for c in cases], cases[0].env, 300, script="rc64_cases.py")


@pytest.mark.parametrize("order", ["real_first", "complex_first"])
def test_einsum_front_end_is_exact_in_either_order(built, order):
    from cudalibrarysamples_amd import torch_einsum
    c = rc.Case("einsum_" + order, dict(m=63, n=45, k=37), ("mk", "kn", "mn"), 0 if order == "real_first" else 1, None)
    A, B, _ = rc.make_inputs(c, False)
    got = torch_einsum.einsum("mk,kn->mn", A.cuda(), B.cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.complex128
    xd.assert_exact(got.cpu(), torch.einsum("mk,kn->mn", A.to(torch.complex128), B.to(torch.complex128)), c.id)
    d = torch_einsum._plans[("mk,kn->mn", (63, 37), (37, 45), A.dtype, False, False, ("dtype_b", B.dtype))].describe()
    assert d["kname"] == rc.KNAME and d["real"] == c.real, d
    # conj_b on the complex second operand / on the real one
    got = torch_einsum.einsum("mk,kn->mn", A.cuda(), B.cuda(), conj_b=True)
    xd.assert_exact(got.cpu(), torch.einsum("mk,kn->mn", A.to(torch.complex128), B.to(torch.complex128).conj()), c.id + " conj_b")
    with pytest.raises(ValueError):
        torch_einsum.einsum("mk,kn->mn", A.cuda(), B.cuda(), compute="32F")
    with pytest.raises(ValueError):
        torch_einsum.einsum("mk,kn->mn", A.cuda().to(torch.float32 if not A.is_complex() else torch.complex64), B.cuda())
    with pytest.raises(RuntimeError):
        torch_einsum.EinsumFunction.apply("mk,kn->mn", A.cuda(), B.cuda())


@pytest.mark.parametrize("mA,mB", xc.LAYOUTS, ids=[xc.LNAME[l] for l in xc.LAYOUTS])
def test_random_data_within_the_fp64_accumulation_bound(env, mA, mB):
    """U(-1, 1), 200 x 136 x 300, alpha = -2 + 1i, beta = 0.5 - 0.5i, against the CPU's complex128 einsum.  Per component the error is at most
    (2 K + 4) 2^-53 mag, mag = (|alpha_r| + |alpha_i|) sum |a| (|b_r| + |b_i|) + (|beta_r| + |beta_i|) (|c_r| + |c_i|): K fp64 accumulation
    steps per component (each product and each sum rounds once) plus the epilogue."""
    import guarded as gd
    ct, ops, h = env
    M, N, K = 200, 136, 300
    real = 0 if mA == "mk" else 1                      # the real tensor: A on two layouts, B on the other two
    c = rc.Case("random_%s_%s" % (mA, mB), dict(m=M, n=N, k=K), (mA, mB, "nm"), real, rc.tiled(real), alpha=rc.ALPHA, beta=rc.BETAS[1])
    gen = torch.Generator().manual_seed(20240 + real)
    dts = c.dtypes()
    A = gd.random_tensor(c.extents(mA), dts[0], gen)
    B = gd.random_tensor(c.extents(mB), dts[1], gen)
    C = gd.random_tensor(c.extents("nm"), "complex128", gen)
    plan = rc.make_plan(ct, ops, h, c)
    try:
        d = plan.describe()
        assert d["kname"] == rc.KNAME and d["real"] == real, d
        pa, pb = xc.Placed(c.extents(mA), dts[0]), xc.Placed(c.extents(mB), dts[1])
        pc, pd = xc.Placed(c.extents("nm"), "complex128"), xc.Placed(c.extents("nm"), "complex128")
        pa.set(A), pb.set(B), pc.set(C)
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        plan.contract(c.alpha, pa.ptr, pb.ptr, c.beta, pc.ptr, pd.ptr, ws.data_ptr(), plan.required_workspace)
        torch.cuda.synchronize()
        got = pd.get()
        pd.check_outside(c.id)
    finally:
        plan.destroy()
    ref = rc.reference(c, A, B, C)
    mag1 = lambda x: (x.real.abs() + x.imag.abs()) if x.is_complex() else x.abs()      # noqa: E731
    mag = (abs(c.alpha.real) + abs(c.alpha.imag)) * torch.einsum("%s,%s->nm" % (mA, mB), mag1(A), mag1(B)) + \
        (abs(c.beta.real) + abs(c.beta.imag)) * mag1(C)
    bound = (2 * K + 4) * 2.0 ** -53 * mag
    err_re, err_im = (got.real - ref.real).abs(), (got.imag - ref.imag).abs()
    print("%s: max error re %.3e im %.3e, smallest bound %.3e, largest error / bound %.3f" % (
        c.id, float(err_re.max()), float(err_im.max()), float(bound.min()), float(torch.maximum(err_re / bound, err_im / bound).max())))
    assert bool((err_re <= bound).all()) and bool((err_im <= bound).all())
