"""Every element-wise and reduction path bit for bit on integer-valued data (the case table, the data and the references are
tests/ew_exact_cases.py; tests/test_ew_exact_cpu.py checks the table on the CPU) — the sibling of tests/test_gpu_exact.py for
cutensorPermute, cutensorElementwiseBinaryExecute, cutensorElementwiseTrinaryExecute and cutensorReduce.

Every case names its kernel with a predicate on the plan's description and runs on at least two draws; MAX / MIN reductions on as many as
it takes for the spikes to visit the ends of the reduced range, both sides of every split boundary and the unrolled loops' tails.  All
tensors live in NaN-filled buffers at the case's element offset and padded pitches; D holds NaN before a launch that reads no C term
(beta = 0: 0 * NaN must not leak), C is D itself or a buffer of its own as the run says.  After each launch: D equals the exact result at
every element (no tolerance, -0 = +0), nothing outside D's elements was written, a separate C is unchanged."""
import pytest

import ew_exact_cases as ec
import exact_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", [c.id for c in ec.CASES])
def test_ew_exact(env, cid):
    ct, ops, h = env
    ec.run_case(ct, ops, h, ec.BY_ID[cid])


def test_ew_exact_on_the_production_libraries(env):
    """the cases that need no switch once more on lib/ (the suite loads lib_hooks/), in one child with its own time limit"""
    xc.in_child(ec.NO_SWITCH, {"CTAMD_LIB_FLAVOUR": "production"}, timeout=600, mode="production", script="ew_exact_cases.py")
