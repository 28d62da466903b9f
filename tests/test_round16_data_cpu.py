"""Proof on the CPU that the rounding regime discriminates (data and rules: tests/rounding_data.py; cases: tests/rounding_cases.py and
tests/rounding_ew.py; tests/test_gpu_round16_exact.py runs the kernels on the same draws).

For every case and draw of the three parts, without a GPU:
  * the bounds hold (integers, the fp32 accumulator exact) and the conditions on the reference hold (the share of outputs that round, at
    most 1 % overflow, for the beta cases at least 64 outputs at which one rounding and two differ);
  * three wrong roundings applied to the exact reference in place of the right one — truncation towards zero, round-half-away-from-zero,
    round-half-up — each differ from what the test expects in at least 16 outputs: a kernel with one of these defects fails the GPU test.
    The beta cases are checked against truncation and against the other type's rule (two roundings for fp16, one for bf16): S + beta * c
    is never an exact tie, so there the two tie rules ARE round-to-nearest; the contraction cases pin them on the same kernels.
    Runs of fewer than 1024 outputs cannot hold 16 such outputs (a reduction to a scalar has one): there every wrong rule must differ
    at least once over the case's draws and runs.  The reductions place an exact tie of each direction in every draw for that
    (rounding_ew.tie_target).  (Round-to-even and truncation agree wherever the nearest value lies towards zero: no data can make a
    wrong rule differ at EVERY output that rounds.)
  * every plan is described on the CPU and checked against its path predicate;
  * over each part and data type at least 1000 exact ties of each kind: to-even-down and to-even-up, of both signs.
rounding_data.round16 itself is checked against numpy's and torch's conversions, which round once."""
import numpy as np
import pytest
import torch

import ew_exact_cases as ew
import exact_cases as xc
import exact_data as xd
import many_mode_cases as mm
import rounding_cases as rc
import rounding_data as rd
import rounding_ew as rw

WRONG = ("trunc", "away", "up")
STATS = []


def told_apart(what, ref, want, dtype, seen, rules=WRONG):
    """every wrong rule, applied to the exact values, gives a result that the comparison with `want` rejects: in 16 outputs or more of
    a run of 1024 outputs or more; `seen` adds up the outputs per rule for all_rules_seen()"""
    ref, want = np.asarray(ref, dtype=np.float64), np.asarray(want, dtype=np.float64)
    for rule in rules:
        differ = int((rd.round16(ref, dtype, rule) != want).sum())
        seen[rule] = seen.get(rule, 0) + differ
        if ref.size >= rd.SMALL:
            assert differ >= rd.MIN_TOLD_APART, "%s: %s differs from the expected result in %d outputs only" % (what, rule, differ)


def all_rules_seen(what, seen, rules=WRONG):
    """over the draws and runs of one case, however small: no wrong rule passes"""
    for rule in rules:
        assert seen.get(rule, 0) >= 1, "%s: %s passes on every draw and run" % (what, rule)


# ---- the rules themselves ---------------------------------------------------------------------------------------------------------------
def test_the_four_rules_on_known_values():
    x = np.array([257.0, -257.0, 259.0, -259.0, 258.5, -258.5, 256.0, 0.0])           # bf16 keeps even integers in [256, 512)
    assert rd.round16(x, "bfloat16", "even").tolist() == [256, -256, 260, -260, 258, -258, 256, 0]
    assert rd.round16(x, "bfloat16", "trunc").tolist() == [256, -256, 258, -258, 258, -258, 256, 0]
    assert rd.round16(x, "bfloat16", "away").tolist() == [258, -258, 260, -260, 258, -258, 256, 0]
    assert rd.round16(x, "bfloat16", "up").tolist() == [258, -256, 260, -258, 258, -258, 256, 0]
    y = np.array([2049.0, 65519.0, 65520.0, -65520.0, 65535.0, 2.0 ** -14 * 3])                 # fp16: 65520 is the tie towards 2^16
    assert rd.round16(y, "float16", "even").tolist() == [2048, 65504, np.inf, -np.inf, np.inf, 2.0 ** -14 * 3]
    assert rd.round16(y, "float16", "trunc").tolist() == [2048, 65504, 65504, -65504, 65504, 2.0 ** -14 * 3]


def test_round_to_nearest_even_is_the_conversion_of_numpy_and_torch():
    rng = np.random.default_rng(16)
    ints = rng.integers(-70000, 70000, 200000).astype(np.float64)
    fine = ints + rd.BETA * (2 * rng.integers(-8, 8, ints.size) + 1)                   # S + beta * c: no value of fp32 for |S| >= 2^10
    with np.errstate(over="ignore"):
        assert np.array_equal(rd.round16(fine, "float16"), fine.astype(np.float16).astype(np.float64))                       # one rounding
        assert np.array_equal(rd.round16(rd.through_fp32(fine), "float16"), fine.astype(np.float32).astype(np.float16).astype(np.float64))
    assert bool((rd.round16(fine, "float16") != rd.round16(rd.through_fp32(fine), "float16")).any())
    for dt in xd.H16:
        assert np.array_equal(rd.round16(ints, dt), xd.round_to(torch.from_numpy(ints), dt).numpy()), dt
        assert np.array_equal(rd.round16(rd.through_fp32(fine), dt), xd.round_to(torch.from_numpy(fine), dt).numpy()), dt


# ---- part 1: contractions ----------------------------------------------------------------------------------------------------------------
def test_the_selection():
    ids = " ".join(c.id for c in rc.ROUNDING)
    for needle in ("h16_4x_aligned", "h16_4p_", "h16_4m_", "h16_4m4_", "h16_8m_", "h16_4q_edges", "ragged_k1000", "sweep_ragged", "_unal_", "unal_padded",
                   "h16p_grid8", "h16_splitk1", "h16_splitk3", "h16_splitk8", "lds_splitk", "gen_77_53_91", "gen_forced", "bf16_gen_off_simple", "_repack"):
        assert needle in ids, needle
    assert len(rc.ROUNDING) > 200 and all(c.dtype in xd.H16 and xd.work(c) < 1e9 for c in rc.ROUNDING)
    left_out = [c.id for c in xc.CASES if c.dtype in xd.H16 and c not in rc.ROUNDING and not c.full_size and xd.work(c) < 1e9]
    assert sorted(left_out) == ["bf16_lone_rounded_sums", "bf16_lone_small_sums", "f16_lone_small_sums"], left_out      # round twice by design


@pytest.mark.parametrize("case", rc.ROUNDING, ids=[c.id for c in rc.ROUNDING])
def test_contraction_draws_round_and_tell_wrong_roundings_apart(case):
    seen = {}
    for swap in (False, True):
        A, B, C = rd.make_rounding(case, swap)
        assert A.dtype == B.dtype == C.dtype == xd.TORCH_DTYPES[case.dtype]
        frac = xd.check_draw(case, A, B, C, swap)                                     # integers; sum |a| |b| max(1, |alpha|) + |beta c| < 2^24
        assert 0 < frac < 0.02
        ref = xd.exact_reference(case, A, B, C)
        want, counts = rd.expected_rounded(case, ref)                                 # asserts the shares
        assert np.array_equal(rd.round16(ref.numpy(), case.dtype), want.numpy())
        told_apart("%s (draw %d)" % (case.id, swap), ref.numpy(), want.numpy(), case.dtype, seen)
        STATS.append(("contraction", case.dtype, case.id, counts))
    all_rules_seen(case.id, seen)


def test_the_signed_operand_changes_sides():
    case = xc.BY_ID["bfloat16_lds_k2048"]
    A0, B0, _ = rd.make_rounding(case, False)
    A1, B1, _ = rd.make_rounding(case, True)
    assert bool((B0 > 0).all()) and bool((A1 > 0).all()) and bool((A0 < 0).any()) and bool((B1 < 0).any())
    assert torch.equal(A0, rd.make_rounding(case, False)[0])
    assert rd.magnitude("bfloat16", 2048) == 5 and rd.magnitude("bfloat16", 7) == 96 and rd.magnitude("bfloat16", 1) == 255 and rd.magnitude("float16", 1) == 256


# ---- part 2: beta below fp32's last place --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.BETA, ids=[c.id for c in rc.BETA])
def test_beta_draws_separate_one_rounding_from_two(case):
    assert case.alpha == 1.0 and case.beta == 2.0 ** -14
    for swap in (False, True):
        A, B, C = rd.make_beta(case, swap)
        c = C.double()
        assert bool((c.abs() <= 15).all()) and bool((c % 2 == 1).all())
        assert 0 < xd.check_draw(case, A, B, C, swap) < 0.02
        ref = xd.exact_reference(case, A, B, C)
        assert bool((ref == contract_plus(case, A, B, C)).all())
        want, counts = rd.expected_beta(case, ref)                                    # asserts: the two rules differ at 64 outputs or more
        contract, other = rd.beta_rules(case, ref)
        assert np.array_equal(want.numpy(), contract)
        told_apart("%s (draw %d)" % (case.id, swap), ref.numpy(), contract, case.dtype, {}, rules=("trunc",))
        assert int((other != contract).sum()) >= rd.MIN_DIFFER and counts[3:7] == [0, 0, 0, 0]
        x = ref.numpy()
        if case.dtype == "float16":                                                   # numpy's fp64 -> fp16 rounds once
            assert np.array_equal(contract, x.astype(np.float16).astype(np.float64))
        else:
            assert np.array_equal(contract, xd.round_to(ref, "bfloat16").numpy())     # fp64 -> fp32 -> bf16: the two roundings


def contract_plus(case, A, B, C):
    """S + beta * c in fp64, S from exact_data.contract_exact: exact, 17 + 14 bits"""
    acc, _ = xd.contract_exact(case, A, B)
    return acc + rd.BETA * C.double()


# ---- part 3: element-wise results and reductions ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def test_the_element_wise_selection():
    ids = " ".join(c.id for c in rw.EW + rw.MM)
    for needle in ("_red_col_add", "_red_row_split_add", "_red_rowany_split_add", "_red_gen_split_mul", "_perm_rowcopy", "_perm_block_vec", "_perm_any_pair",
                   "_perm_transpose_w256", "bf16_perm_transpose_narrow", "f16_perm_transpose_narrow_pad", "_bin_rowcopy_pad_add", "_bin_any_mul", "_tri_two_pass_add_add", "_tri_two_pass_mul_add", "_tri_two_pass_add_mul",
                   "bf16_perm_rev12", "f16_perm_rev12", "bf16_bin_mixed9_add", "bf16_red_alt10_add"):
        assert needle in ids, needle
    every = [c for c in ew.CASES + mm.CASES if c.dtype in xd.H16]
    assert all(c in rw.EW + rw.MM or any(o in ("MAX", "MIN") for o in rw._ops(c)) for c in every)          # only MAX / MIN stay out
    assert sum(1 for c in rw.EW if c.env) == 4, [c.id for c in rw.EW if c.env]                              # the LANES_ONLY transpositions
    for c in rw.EW + rw.MM:
        for scal, _ in rw.runs(c):
            assert all(abs(s) in ((0.0, 1.0, 2.0, 3.0) if c.kind in ("permutation", "binary") else (1.0, 2.0)) or (c.kind == "reduction" and s == 0.0)
                       for s in scal), (c.id, scal)


@pytest.mark.parametrize("case", rw.EW + rw.MM, ids=[c.id for c in rw.EW + rw.MM])
def test_element_wise_draws_round_and_tell_wrong_roundings_apart(lib, case):
    ct, ops, h = lib
    d = (mm if case in rw.MM else ew).plan_path(ct, ops, h, case)                     # the plan is on the path the case names
    assert ew.n_draws(case, d) == 2
    seen = {}
    for draw in range(2):
        ins = rw.make_draw(case, draw, d)
        for run in rw.runs(case):
            assert 0 < rw.check_draw(case, ins, run, d) < 1
            ref = ew.reference(case, ins, run)
            want = rw.expected(case, ref)                                             # asserts the share; keeps the counts in rw.STATS
            assert np.array_equal(rd.round16(ref, case.dtype), want.numpy())
            told_apart("%s (draw %d, %s)" % (case.id, draw, run), ref, want.numpy(), case.dtype, seen)
            STATS.append(rw.STATS[-1])
    all_rules_seen(case.id, seen)


# ---- plans -----------------------------------------------------------------------------------------------------------------------------------
def test_every_contraction_plans_onto_its_path(lib):
    ct, ops, h = lib
    for case in rc.ROUNDING + rc.BETA:
        if case.group is None:
            xc.plan_path(ct, ops, h, case)


@pytest.mark.parametrize("group", rc.ROUNDING_GROUPS)
def test_every_switched_contraction_plans_onto_its_path(lib, group):
    cases = [c for c in rc.ROUNDING if c.group == group]
    xc.in_child([c.id for c in cases], cases[0].env, timeout=300, mode="plan")


@pytest.mark.parametrize("group", [g for g in rc.BETA_GROUPS if g != "in_process"])
def test_every_switched_beta_case_plans_onto_its_path(lib, group):
    cases = [c for c in rc.BETA if c.group == group]
    assert all(c.env == cases[0].env for c in cases)
    rc.in_child([c.id for c in cases], cases[0].env, timeout=300, mode="plan_beta")


# ---- the ties of the whole module (after the draws above) ------------------------------------------------------------------------------------
def test_ties_of_both_signs_and_directions():
    parts = [p for p, n in (("contraction", 2 * len(rc.ROUNDING)), ("elementwise", 2 * len(rw.EW + rw.MM))) if sum(1 for s in STATS if s[0] == p) >= n]
    rep = rd.check_ties(STATS, parts=parts)
    for p in parts:
        for dt in xd.H16:
            assert rep[(p, dt)][1] >= (rd.MIN_ROUNDING if p == "contraction" else rw.MIN_ROUNDING)
