"""The exact-data generator, reference and comparator (tests/exact_data.py) on the CPU, for the case table of tests/test_gpu_exact.py.

- Every case that fits the CPU (all but the full-size ones): both draws hold integers only, the dense operand has no zero, every contracted
  index is live in the other operand, the accumulator bound holds, and at most 1 % of the exact outputs (none for 32- and 64-bit types)
  are not values of the output type.  The 4098^3 / 4100^3 cases check the last condition on 4096 sampled outputs (int64 dot products).
- The oracle's literal fp32 loop (acc64=False) and its 16-bit entry points return exactly the integer reference on this data: a second
  summation order gives the same bits, and the oracle's 16-bit rounding is pinned.
- Why the exact tests exist: with one product removed from one output, the tolerance tests' comparison still passes, assert_exact fails."""
import numpy as np
import pytest
import torch

import exact_cases as xc
import exact_data as xd
import oracle
from util import assert_close

ON_CPU = [c for c in xc.CASES if not c.full_size and c.kind == "contraction" and c.data_key == c.id]
HUGE = 2e10          # multiply-adds beyond which the CPU checks sampled outputs only


def _sampled(case, A, B, C):
    """4096 outputs of a large case as int64 dot products -> exact values (alpha, beta applied)"""
    m = xd.Modes(*case.modes[:3])
    rng = np.random.default_rng(5)
    pa, pb = xd._planes(A), xd._planes(B)
    idx = [rng.integers(0, case.ext[c], xd.SAMPLES) for c in m.C]
    out = []
    for s in range(xd.SAMPLES):
        at = {c: int(idx[i][s]) for i, c in enumerate(m.C)}
        sa = tuple(at[c] if c in at else slice(None) for c in m.A)
        sb = tuple(at[c] if c in at else slice(None) for c in m.B)
        ra, rb = "".join(c for c in m.A if c not in at), "".join(c for c in m.B if c not in at)
        acc = float(np.einsum("%s,%s->" % (ra, rb), pa[0][sa], pb[0][sb]))
        out.append(case.alpha * acc + case.beta * float(C[tuple(at[c] for c in m.C)]))
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("case", ON_CPU, ids=[c.id for c in ON_CPU])
def test_draws_hold_the_invariants(case):
    for swap in (False, True):
        A, B, C = xd.make_exact(case, swap)
        assert A.dtype == B.dtype == C.dtype == xd.TORCH_DTYPES[case.dtype]
        frac = xd.check_draw(case, A, B, C, swap)
        assert 0 < frac < 1
        if xd.work(case) > HUGE:
            ref = _sampled(case, A, B, C)
        else:
            ref = xd.exact_reference(case, A, B, C)
        want, share = xd.expected(case, ref)          # asserts the share of outputs that round
        parts = torch.view_as_real(ref) if ref.is_complex() else ref
        assert bool((2 * parts == (2 * parts).round()).all())                 # integers, or halves where alpha / beta is a half
        if case.dtype in xd.H16 and not case.dense_values:
            assert float(ref.abs().max()) <= 2 * 6 * 32 + 6, "16-bit sums beyond six sigma: %r" % float(ref.abs().max())


@pytest.fixture(scope="module")
def lib(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops


def test_every_case_plans_onto_its_path(lib):
    """the planner needs no GPU: every case of the table is on the path it covers (what only a device shows is left to the GPU run)"""
    ct, ops = lib
    h = ops.Handle()
    for case in xc.CASES:
        if case.group is None:
            xc.plan_path(ct, ops, h, case)


@pytest.mark.parametrize("group", xc.GROUPS)
def test_every_switched_case_plans_onto_its_path(lib, group):
    ct, ops = lib
    cases = [c for c in xc.CASES if c.group == group]
    xc.in_child([c.id for c in cases], cases[0].env, timeout=300, mode="plan")


def test_block_sparse_draws():
    case = xc.BY_ID["f64_blocksparse"]
    for swap in (False, True):
        dense, lay, A, B, C, frac = xc.blocksparse_inputs(case, swap)
        assert 0 < frac < 1
        xd.expected(dense, xd.exact_reference(dense, A, B, C))


def test_the_two_draws_differ_and_are_reproducible():
    case = xc.BY_ID["bfloat16_lds_k2048"]
    A0, B0, _ = xd.make_exact(case, False)
    A1, B1, _ = xd.make_exact(case, True)
    assert bool((A0 != 0).all()) and bool((B1 != 0).all())                         # the dense operand changes sides
    assert 0.2 < float((B0 != 0).double().mean()) < 0.8 and 0.2 < float((A1 != 0).double().mean()) < 0.8   # K = 2048: density 1/2
    A0b, B0b, _ = xd.make_exact(case, False)
    assert torch.equal(A0, A0b) and torch.equal(B0, B0b)


def test_sixteen_bit_lone_mode_sums_are_rounded_once_where_they_leave_the_exact_range():
    """bf16_lone_small_sums: the lone-mode sums are integers of [-7, 7], rounding them changes nothing.  bf16_lone_rounded_sums: sums of
    about 600, where bf16 keeps multiples of 4 — the reference rounds them, and that changes the result."""
    small, big = xc.BY_ID["bf16_lone_small_sums"], xc.BY_ID["bf16_lone_rounded_sums"]
    for case, changes in ((small, False), (big, True)):
        A, B, C = xd.make_exact(case)
        s = A.double().sum(dim=case.modes[0].index("j"))
        assert (float(s.abs().max()) > 256) == changes
        assert bool((xd.round_to(s, case.dtype) != s).any()) == changes
        unrounded = case.alpha * torch.einsum("kji,lk->li", A.double(), B.double()) + case.beta * C.double()
        assert bool((xd.exact_reference(case, A, B, C) != unrounded).any()) == changes


SMALL = ["f32_unal_mk_kn_50x50x50", "f32_unal_km_nk_131x67x191", "f32_rows_mk_nk_batch", "f32_rows_multi", "f32_short_k_batch", "f32_lone_A",
         "float64_gen_77_53_91", "complex64_gen_conjA", "complex128_gen_conjB", "complex64_gen_batch"]


@pytest.mark.parametrize("cid", SMALL)
def test_oracle_fp32_loop_returns_the_integers(cid):
    """oracle.contract(acc64=False): the literal loop nest in the data type's own accumulator, in loop order — a second summation order"""
    case = xc.BY_ID[cid]
    A, B, C = xd.make_exact(case)
    want, _ = xd.expected(case, xd.exact_reference(case, A, B, C))
    f = lambda t: np.asfortranarray(t.numpy())   # noqa: E731
    D = np.zeros_like(f(C))
    oracle.contract(f(A), case.modes[0], f(B), case.modes[1], D, case.modes[2], alpha=case.alpha, beta=case.beta, C=f(C), acc64=False,
                    conjA=case.conjA, conjB=case.conjB)
    xd.assert_exact(torch.from_numpy(np.ascontiguousarray(D)), want, cid)


@pytest.mark.parametrize("cid", ["bfloat16_h16_4x_aligned_mk_kn", "float16_h16_4x_aligned_km_kn", "bfloat16_lds_splitk_ragged", "float16_lds_k2048",
                                 "bf16_lds_splitk_odd", "bfloat16_h16_4q_unal_mk_kn_300x204x100"])
def test_oracle_16_bit_entry_points_return_the_rounded_integers(cid):
    case = xc.BY_ID[cid]
    kind = "bf16" if case.dtype == "bfloat16" else "f16"
    for swap in (False, True):
        A, B, C = xd.make_exact(case, swap)
        want, _ = xd.expected(case, xd.exact_reference(case, A, B, C))
        bits = lambda t: np.asfortranarray(t.view(torch.int16).numpy().view(np.uint16))   # noqa: E731
        D = np.zeros_like(bits(C))
        oracle.contract(bits(A), case.modes[0], bits(B), case.modes[1], D, case.modes[2], alpha=case.alpha, beta=case.beta, C=bits(C), h16=kind)
        xd.assert_exact(torch.from_numpy(oracle.from_bits(D, kind)), want, cid)


def test_one_lost_product_passes_the_tolerance_and_fails_the_exact_compare():
    """The headline's extents (K = 64^3, every product in {1 .. 9}): one product removed from one output is far inside rtol 1e-4 — the
    tolerance of tests/test_gpu_contraction.py::test_headline_einsum_full_size — and fails assert_exact with the product as the difference.
    (A thinned draw of the same K on the CPU: 8 x 8 outputs.)"""
    case = xc.Case("headline_thin", "float32", dict(xc.HEADLINE, a=8, e=8), xc.HEAD_MODES)
    A, B, C = xd.make_exact(case)
    xd.check_draw(case, A, B, C)
    ref = xd.exact_reference(case, A, B, C)
    # the U(0, 1) data of the tolerance test gives outputs of about K / 4; here |sum| ~ 4.7 sqrt(K): compare at the tolerance test's scale
    scale = torch.full_like(ref, 64.0 ** 3 / 4)
    hurt = (ref + scale).clone()
    hurt[3, 5] -= float(A[0, 0, 0, 5] * B[3, 0, 0, 0])
    assert_close(hurt.numpy(), (ref + scale).numpy(), rtol=1e-4, what="one product lost")
    with pytest.raises(AssertionError, match=r"1 of 64 elements differ"):
        xd.assert_exact(hurt, ref + scale)
    xd.assert_exact(ref + scale, ref + scale)


def test_one_lost_product_passes_the_16_bit_tolerance_and_fails_the_exact_compare():
    """bf16 at K = 8192, rtol 8e-3 / atol 0.15 (tests/test_gpu_h16.py::test_full_size_8192_sampled, mean |product| 0.25 there): a lost
    product of that size passes; on the exact data a lost product is +-1 and fails."""
    case = xc.Case("bf16_k8192_thin", "bfloat16", dict(m=64, n=64, k=8192), ("mk", "kn", "mn"))
    A, B, C = xd.make_exact(case)
    xd.check_draw(case, A, B, C)
    ref = xd.exact_reference(case, A, B, C)
    want, share = xd.expected(case, ref)
    assert share == 0.0
    rng = np.random.default_rng(3)
    real = (rng.random((64, 8192)) * 2 - 1) @ (rng.random((8192, 64)) * 2 - 1)            # the tolerance test's data
    big = np.argwhere(np.abs(real) > 20)[0]                                                  # an output of typical size (sigma = 30)
    lost = real.copy()
    lost[tuple(big)] -= 0.25 * np.sign(real[tuple(big)])
    assert_close(lost, real, rtol=8e-3, atol=0.15, what="one product lost")
    k = int(torch.nonzero(B[:, 9])[0])
    hurt = ref.clone()
    hurt[7, 9] -= float(A[7, k] * B[k, 9])
    with pytest.raises(AssertionError, match=r"1 of 4096 elements differ"):
        xd.assert_exact(xd.round_to(hurt, "bfloat16"), want)


def test_assert_exact_reports_the_difference_and_takes_signed_zeros():
    a = torch.tensor([0.0, 1.0, -3.0])
    xd.assert_exact(torch.tensor([-0.0, 1.0, -3.0]), a)
    with pytest.raises(AssertionError, match=r"got - expected = -2.0"):
        xd.assert_exact(torch.tensor([0.0, -1.0, -3.0]), a)
    with pytest.raises(AssertionError, match=r"1 of 3"):
        xd.assert_exact(torch.tensor([0.0, float("nan"), -3.0]), a)
