"""Unary operators on element-wise and reduction operands, bit for bit (the case table, the data and the references are
tests/unary_cases.py; tests/test_unary_cpu.py checks the table on the CPU): ABS, NEG, RELU, SQRT and RCP on data that makes every correct
evaluation exact, on every real-data geometry of tests/ew_exact_cases.py — hence every element-wise kernel and every reduction variant
with and without a split — in NaN-guarded buffers at the base case's element offset and padded pitches.

After each launch: D equals the exact result at every element (no tolerance), nothing outside D's elements was written, a separate C is
unchanged.  D holds NaN before a launch that reads no C term — also where C carries an operator."""
import numpy as np
import pytest

import ew_exact_cases as ec
import exact_cases as xc
import unary_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", [c.id for c in uc.CASES])
def test_unary_exact(env, cid):
    ct, ops, h = env
    uc.run_case(ct, ops, h, uc.BY_ID[cid])


@pytest.mark.parametrize("bid", ["f32_perm_transpose_t64", "bf16_perm_transpose_w256", "f64_bin_transpose_add", "f32_tri_two_tiles_64_add_add",
                                 "f32_red_col_split_max", "bf16_red_row_max", "f32_red_rowany_split_add"])
def test_the_operator_picks_the_kernel_twin(env, bid):
    """a run on the ABS plan, then on the identity plan of the same geometry, then on the ABS plan again, on one handle and the same signed
    data: each gives its own exact result, and the two differ — the plan memo and the twin selection go by the operator"""
    ct, ops, h = env
    base = ec.BY_ID[bid]
    with_op = uc.UCase(base, dict(A="ABS"), "abs")
    ident = uc.UCase(base, {}, "identity")
    d = uc.plan_path(ct, ops, h, with_op)
    assert d == dict(uc.plan_path(ct, ops, h, ident), unary=[ct.OP_ABS, ct.OP_IDENTITY, ct.OP_IDENTITY])
    ins = uc.make_draw(with_op, 0, d)
    assert ins["A"].min() < 0                                                      # signed data: |a| != a somewhere
    assert all(np.array_equal(x, uc.make_draw(ident, 0, d)[t]) for t, x in ins.items())      # ... and the same data for both plans
    run = base.runs[0]
    assert not np.array_equal(uc.reference(with_op, ins, run), uc.reference(ident, ins, run))
    for case in (with_op, ident, with_op):
        plan = uc.make_plan(ct, ops, h, base, case.un)
        try:
            uc.run_plan(ct, plan, case, d, case.id)
        finally:
            plan.destroy()


def test_unary_exact_on_the_production_libraries(env):
    """the cases that need no switch once more on lib/ (the suite loads lib_hooks/), in one child with its own time limit"""
    xc.in_child(uc.NO_SWITCH, {"CTAMD_LIB_FLAVOUR": "production"}, timeout=600, mode="production", script="unary_cases.py")
