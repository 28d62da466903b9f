"""Type conversion in cutensorPermute and the binary form, bit for bit on integer-valued data (the case table, the plans and the runner
are tests/convert_cases.py; tests/test_convert_cpu.py checks the table on the CPU): every pair on the converting row copy, the
converting transposition at every tile width and the converting element-gather kernel, with and without the C term.

Every case names its kernel with a predicate on the plan's description (variant and "convert") and runs on two draws.  All tensors live
in NaN-filled buffers of their own data type at the case's element offset and padded pitches; D holds NaN before a launch that reads no C
term, C is D itself or a buffer of its own as the run says.  After each launch: D equals the exact result at every element (no tolerance),
nothing outside D's elements was written, A and a separate C are unchanged.  The data never rounds: tests/test_gpu_convert_rounding.py
is about the rounding."""
import pytest

import convert_cases as cc
import exact_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", [c.id for c in cc.CASES])
def test_convert_exact(env, cid):
    ct, ops, h = env
    cc.run_case(ct, ops, h, cc.BY_ID[cid])


def test_padded_converting_permutation(env):
    """fp32 -> bf16 with CUTENSOR_OPERATION_DESCRIPTOR_PADDING_*: the border holds the pad value in D's type, at D's element size"""
    ct, ops, h = env
    cc.run_padding(ct, ops, h)


def test_convert_exact_on_the_production_libraries(env):
    """the cases once more on lib/ (the suite loads lib_hooks/), in one child with its own time limit"""
    xc.in_child(cc.NO_SWITCH, {"CTAMD_LIB_FLAVOUR": "production"}, timeout=600, mode="production", script="convert_cases.py")
