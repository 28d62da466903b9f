"""cutensorContractTrinary, cutensorBlockSparseContract and the padded cutensorPermute bit for bit on integer-valued data in guarded buffers
(the case table, the data rule and the references are tests/composite_cases.py; tests/test_composite_cpu.py checks the table on the CPU) —
the sibling of tests/test_gpu_exact.py and tests/test_gpu_ew_exact.py for the entry points that split one call into several launches.

Every case names its path with a predicate on the plan's description and runs on two draws, once per place of its beta source.  All
tensors live in 0xFF-filled buffers at the case's element offset and padded pitches, the workspace is exactly required_workspace bytes
between guards.  After each launch: the output equals the exact result at every element (no tolerance), nothing outside the output's
elements was written, the workspace's guards hold, and every input and a separate beta source are unchanged byte for byte."""
import pytest

import composite_cases as cc
import exact_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", [c.id for c in cc.CASES])
def test_composite_exact(env, cid):
    ct, ops, h = env
    cc.run_case(ct, ops, h, cc.BY_ID[cid])


def test_composite_exact_on_the_production_libraries(env):
    """the cases that need no switch once more on lib/ (the suite loads lib_hooks/), in one child with its own time limit"""
    xc.in_child(cc.NO_SWITCH, {"CTAMD_LIB_FLAVOUR": "production"}, timeout=600, mode="production", script="composite_cases.py")
