"""cutensorElementwiseTrinaryExecute on complex64 / complex128 tensors, bit for bit on integer-valued data (the case table, the plans and
the runner are tests/cplx_trinary_cases.py; tests/test_cplx_trinary_cpu.py checks the table on the CPU): the E form on the transposing,
the row-copy and the gather kernel, the two-tile form, the two-pass form with its in-place launch, conjugation in every role, gamma = 0
over a NaN C.

Every case names its path with a predicate on the plan's description and runs on two draws.  All tensors live in NaN-filled buffers at the
case's element offset and padded pitches.  After each launch: D equals the exact result at every element (no tolerance), nothing outside
D's elements was written, A, B and a separate C are unchanged."""
import pytest

import cplx_trinary_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", [c.id for c in tc.CASES])
def test_cplx_trinary_exact(env, cid):
    ct, ops, h = env
    tc.run_case(ct, ops, h, tc.BY_ID[cid])
