"""Contractions with a mode that ONE input carries and nothing else ('ijk,kl->il': j) — VERDICT r5 "Missing #4".  The reference's N-ary
front end builds exactly such pairwise steps: _compute_target_tensor drops every mode no later operand or the target needs
(cuTENSOR/python/cutensor/torch/einsum.py:111-156), and torch.einsum, the reference's comparator, accepts the equation.  The engine reduces
the operand over the mode first (cutensorReduce into a temporary in the workspace), then contracts (csrc/host/contraction_route.cpp split_lone_modes).

Through the C ABI against the oracle (fp32 rtol 1e-4 on U(0,1) data; fp16 rtol 2e-3; complex64 rtol 1e-4), through the engine's PyTorch
front end with gradients against torch.einsum at the tolerance of einsum_test.py:35-42 (rtol 5e-3 / atol 6e-3), and through the reference's
own unmodified binding."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return torch, ct, ops, ops.Handle()


CASES = [  # equation (row-major framework form), shapes
    ("ijk,kl->il", (33, 7, 50), (50, 21)),          # the review's example: j lives in A alone
    ("ij,jk->k", (40, 50), (50, 31)),               # i lives in A alone, the result is a vector
    ("ik,jkl->ij", (20, 50), (17, 50, 9)),          # l lives in B alone
    ("aij,kbj->ik", (5, 30, 50), (12, 6, 50)),      # one lone mode in each operand
    ("ij,kl->", (6, 7), (8, 9)),                    # everything is summed: product of two full reductions
    ("bij,bjk->bk", (4, 10, 50), (4, 50, 13)),      # with a batch mode
]


# rtol of one call and of the alpha / beta call: fp32 / complex64 as before (oracle); bf16: the temporary and the output are each rounded to
# 8 bits (2 x 2^-9, tests/test_gpu_h16_unaligned.py's 8e-3); fp64 / complex128 1e-12
RTOL = {"float32": (1e-4, 1e-4), "float16": (2e-3, 3e-3), "complex64": (1e-4, 1e-4), "bfloat16": (8e-3, 8e-3), "float64": (1e-12, 1e-12),
        "complex128": (1e-12, 1e-12)}


def _rounded(rng, shape, dtype, torch):
    """U(0, 1) (complex: both parts) rounded once to the data type, as (numpy copy in a type numpy has, device tensor)"""
    x = rng.random(shape)
    if dtype.startswith("complex"):
        x = x + 1j * rng.random(shape)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(getattr(torch, dtype))
    return (t.to(torch.float32) if dtype == "bfloat16" else t).numpy(), t.cuda()


@pytest.mark.parametrize("dtype", ["float32", "float16", "complex64", "bfloat16", "float64", "complex128"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_lone_modes_through_the_c_abi_against_the_oracle(env, case, dtype):
    import oracle
    torch, ct, ops, h = env
    eq, sa, sb = case
    rng = np.random.default_rng(abs(hash((eq, dtype))) % 1000)
    a, dA = _rounded(rng, sa, dtype, torch)
    b, dB = _rounded(rng, sb, dtype, torch)
    p = oracle.einsum_parse(eq, sa, sb)
    assert p is not None
    cdt = {"float32": ct.R_32F, "float16": ct.R_16F, "complex64": ct.C_32F, "bfloat16": ct.R_16BF, "float64": ct.R_64F, "complex128": ct.C_64F}[dtype]
    plan = ops.contraction_plan(h, p["extentA"], p["modesA"], p["extentB"], p["modesB"], p["extentC"], p["modesC"], dtype=cdt, workspace_limit=1 << 28)
    d = plan.describe()
    assert d.get("lone_reduce_A", 0) + d.get("lone_reduce_B", 0) >= 1, d
    assert plan.required_workspace >= 256 and plan.required_workspace <= plan.workspace_estimate + (1 << 20)
    out = torch.full(p["output_shape"] or [1], float("nan"), dtype=dA.dtype, device="cuda")
    ws = torch.empty(plan.required_workspace, dtype=torch.uint8, device="cuda")
    plan.contract(1.0, dA.data_ptr(), dB.data_ptr(), 0.0, out.data_ptr(), out.data_ptr(), ws.data_ptr(), plan.required_workspace)
    torch.cuda.synchronize()
    wide = np.complex128 if dtype.startswith("complex") else np.float64
    got = out.cpu().to(torch.float32 if dtype == "bfloat16" else out.dtype).numpy().reshape(p["output_shape"])
    if dtype in ("float32", "complex64"):
        want = oracle.einsum(eq, a, b)
        np.testing.assert_allclose(got, want, rtol=RTOL[dtype][0])
    else:
        # 16-bit: the temporary is rounded to the data type once more than a fused sum would be: rtol 2 x half an ulp + the output's own
        want = np.einsum(eq, a.astype(wide), b.astype(wide))
        np.testing.assert_allclose(got.astype(wide), want, rtol=RTOL[dtype][0])
    # alpha / beta ride on the inner contraction
    c0h, c0 = _rounded(rng, p["output_shape"] or [1], dtype, torch)
    out2 = c0.clone()
    plan.contract(0.5, dA.data_ptr(), dB.data_ptr(), 2.0, c0.data_ptr(), out2.data_ptr(), ws.data_ptr(), plan.required_workspace)
    torch.cuda.synchronize()
    want2 = 0.5 * np.einsum(eq, a.astype(wide), b.astype(wide)) + 2.0 * c0h.astype(wide).reshape(p["output_shape"])
    np.testing.assert_allclose(out2.cpu().to(torch.float32 if dtype == "bfloat16" else out2.dtype).numpy().reshape(p["output_shape"]), want2,
                               rtol=RTOL[dtype][1])
    plan.destroy()


def test_long_zero_mean_lone_mode_in_fp16(env):
    """The other side of the fp16 temporary's scale: zero-mean A (|a| <= 4e-3) over j = 100 000.  The sum grows like sqrt(j) (~0.7), and the
    scaled temporary must stay in fp16's normal range (2^-14 and up) so that it is as precise as an unscaled one.  Each element of D is
    checked against its own error bound: 2 x 2^-11 of sum_k |T[i, k]| |b[k, l]| (T the exact sum over j) — a temporary scaled by
    2^-ceil(log2 j) sits in the subnormals here and misses it."""
    torch, ct, ops, h = env
    eq, sa, sb = "ijk,kl->il", (6, 100000, 8), (8, 5)
    g = torch.Generator()
    g.manual_seed(4)
    A = ((torch.rand(sa, generator=g, dtype=torch.float64) * 2 - 1) * 4e-3).to(torch.float16)
    B = (torch.rand(sb, generator=g, dtype=torch.float64) + 0.5).to(torch.float16)
    T = A.double().sum(1)
    want = T @ B.double()
    bound = 2 * 2.0 ** -11 * (T.abs() @ B.double().abs()) + 2.0 ** -24
    plan = ops.contraction_plan(h, list(reversed(sa)), "kji", list(reversed(sb)), "lk", [5, 6], "li", dtype=ct.R_16F)
    assert plan.describe()["lone_reduce_A"] == 1, plan.describe()
    dA, dB = A.cuda(), B.cuda()
    out = torch.full((6, 5), float("nan"), dtype=torch.float16, device="cuda")
    ws = torch.empty(max(plan.required_workspace, 1), dtype=torch.uint8, device="cuda")
    plan.contract(1.0, dA.data_ptr(), dB.data_ptr(), 0.0, out.data_ptr(), out.data_ptr(), ws.data_ptr(), plan.required_workspace)
    torch.cuda.synchronize()
    err = (out.cpu().double() - want).abs()
    assert bool((err <= bound).all()), (float((err / bound).max()), err, bound)
    plan.destroy()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_long_lone_mode_in_16_bit_data(env, dtype):
    """'ijk,kl->il' with j = 100 000 and A in [0.5, 1.5]: the sum over j (~1e5) is far beyond fp16's 65504 while the contracted result
    (|b| ~ 1e-3) is ~800.  The fp16 temporary holds the sum scaled by 2^-ceil(log2(j) / 2) and the inner contraction's alpha scales it back
    (csrc/host/create_plan.cpp, loneShiftA); bf16 has the range, this is its precision over a long lone mode.  Against fp64 on the rounded inputs
    at the tolerances of the test above."""
    torch, ct, ops, h = env
    eq, sa, sb = "ijk,kl->il", (6, 100000, 8), (8, 5)
    g = torch.Generator()
    g.manual_seed(3)
    tdt = getattr(torch, dtype)
    A = (torch.rand(sa, generator=g, dtype=torch.float64) + 0.5).to(tdt)
    B = (torch.rand(sb, generator=g, dtype=torch.float64) * 1e-3 + 5e-4).to(tdt)
    want = torch.einsum(eq, A.double(), B.double())
    assert float(A.double().sum(1).max()) > 65504.0 and float(want.abs().max()) < 2000.0
    cdt = ct.R_16F if dtype == "float16" else ct.R_16BF
    # cuTENSOR modes are the row-major ones reversed (first mode fastest)
    plan = ops.contraction_plan(h, list(reversed(sa)), "kji", list(reversed(sb)), "lk", [5, 6], "li", dtype=cdt)
    assert plan.describe()["lone_reduce_A"] == 1, plan.describe()
    dA, dB = A.cuda(), B.cuda()
    out = torch.full((6, 5), float("nan"), dtype=tdt, device="cuda")
    ws = torch.empty(max(plan.required_workspace, 1), dtype=torch.uint8, device="cuda")
    for alpha, beta in ((1.0, 0.0), (0.5, 2.0)):
        plan.contract(alpha, dA.data_ptr(), dB.data_ptr(), beta, out.data_ptr(), out.data_ptr(), ws.data_ptr(), plan.required_workspace)
        torch.cuda.synchronize()
        got = out.cpu().double()
        assert bool(torch.isfinite(got).all()), got
        ref = want if beta == 0.0 else alpha * want + beta * ref_prev
        torch.testing.assert_close(got, ref, rtol=2e-3 if dtype == "float16" else 8e-3, atol=0.0)
        ref_prev = got
    plan.destroy()


@pytest.mark.parametrize("dtype", ["float32", "float16", "complex64"])
def test_front_end_with_gradients_and_an_n_ary_chain(env, dtype):
    """te.einsum / EinsumFunction (forward + both gradients: d_b = einsum(A, C -> B) has the lone mode again, d_a broadcasts over it) and an
    EinsumGeneral chain whose first pairwise step drops a mode — against torch.einsum at einsum_test.py:35-42's tolerance."""
    torch, ct, ops, h = env
    from cudalibrarysamples_amd import torch_einsum as te
    tdt = getattr(torch, dtype)
    torch.manual_seed(0)
    scale = 0.25 if dtype == "float16" else 1.0
    tol = dict(rtol=5e-3, atol=6e-3)
    for eq, sa, sb in (("ijk,kl->il", (20, 6, 50), (50, 30)), ("ij,jk->k", (30, 50), (50, 20))):
        a = (torch.randn(sa, device="cuda", dtype=tdt) * scale).requires_grad_(True)
        b = (torch.randn(sb, device="cuda", dtype=tdt) * scale).requires_grad_(True)
        out = te.EinsumFunction.apply(eq, a, b)
        ref = torch.einsum(eq, a.detach().to(torch.complex128 if tdt.is_complex else torch.float64), b.detach().to(torch.complex128 if tdt.is_complex else torch.float64))
        torch.testing.assert_close(out.detach().to(ref.dtype), ref, **tol)
        g = torch.randn_like(out) * scale
        out.backward(g)
        a2 = a.detach().clone().requires_grad_(True)
        b2 = b.detach().clone().requires_grad_(True)
        torch.einsum(eq, a2.float() if dtype == "float16" else a2, b2.float() if dtype == "float16" else b2).backward(g.float() if dtype == "float16" else g)
        torch.testing.assert_close(a.grad.to(a2.grad.dtype), a2.grad, **tol)
        torch.testing.assert_close(b.grad.to(b2.grad.dtype), b2.grad, **tol)
    x = torch.randn(12, 5, 40, device="cuda", dtype=tdt) * scale
    y = torch.randn(40, 16, device="cuda", dtype=tdt) * scale
    z = torch.randn(16, 9, device="cuda", dtype=tdt) * scale
    got = te.EinsumGeneral("ijk,kl,lm->im", x, y, z)
    wide = torch.complex128 if tdt.is_complex else torch.float64
    torch.testing.assert_close(got.to(wide), torch.einsum("ijk,kl,lm->im", x.to(wide), y.to(wide), z.to(wide)), rtol=5e-3, atol=6e-2 if dtype == "float16" else 6e-3)


def test_reference_binding_runs_lone_mode_steps(built):
    """The reference's unmodified binding + python package (oracle/_ref/pyref): EinsumFunction on 'ijk,kl->il' / 'ij,jk->k' and an
    EinsumGeneral chain that produces such a step (its binding used to dereference a null plan here: NOTES.md section 5c)."""
    import glob
    import torch
    pyref = os.path.join(ROOT, "oracle", "_ref", "pyref")
    if not glob.glob(os.path.join(pyref, "cutensor", "torch", "binding*.so")):
        pytest.skip("oracle/_ref/pyref was not built (reference tree absent at build time)")
    for p in (pyref, os.path.join(ROOT, "tests", "sample_compat", "pyshim")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import cutensor.torch as rct
    torch.manual_seed(0)
    tol = dict(rtol=5e-3, atol=6e-3)
    for tdt in (torch.float32, torch.float16, torch.complex64):
        s = 0.25 if tdt == torch.float16 else 1.0
        a = torch.randn(20, 6, 50, device="cuda", dtype=tdt) * s
        b = torch.randn(50, 30, device="cuda", dtype=tdt) * s
        wide = torch.complex128 if tdt.is_complex else torch.float64
        torch.testing.assert_close(rct.EinsumFunction.apply("ijk,kl->il", a, b).to(wide), torch.einsum("ijk,kl->il", a.to(wide), b.to(wide)), **tol)
        a2 = torch.randn(30, 50, device="cuda", dtype=tdt) * s
        torch.testing.assert_close(rct.EinsumFunction.apply("ij,jk->k", a2, b).to(wide), torch.einsum("ij,jk->k", a2.to(wide), b.to(wide)), **tol)
        z = torch.randn(30, 9, device="cuda", dtype=tdt) * s
        torch.testing.assert_close(rct.EinsumGeneral("ijk,kl,lm->im", a, b, z).to(wide), torch.einsum("ijk,kl,lm->im", a.to(wide), b.to(wide), z.to(wide)),
                                   rtol=5e-3, atol=6e-2 if tdt == torch.float16 else 6e-3)
