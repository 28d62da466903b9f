"""The workspace contract on the MI355X, for every case of tests/workspace_cases.py: D inside a NaN guard with a padded pitch, a
workspace of exactly required_workspace bytes between 0xFF guards (tests/guarded.py), alpha != 1, beta = 0 and beta != 0; D against
fp64 / complex128 at the family tests' tolerances, no store outside D or the workspace body, the same bits from a workspace that held
zeros (nothing reads a partial slot or temporary that nothing wrote), required - 1 bytes refused with D untouched; then the plan at the
MIN estimate (the reference binding's retry path).  The cases that need no hooks switch run once more on the production libraries
(lib/) in a child process."""
import pytest

from workspace_cases import CASES, NO_HOOKS, in_child, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_workspace_contract(env, case):
    ct, ops, h = env
    if case.fresh:   # a switch the library reads once per process: a child process started with it
        in_child("run", [case.id], case.env, timeout=300)
    else:
        run_case(ct, ops, h, case)


def test_workspace_contract_on_the_production_libraries(built):
    """bench.py, smoke() and the samples load lib/, whose host code is built without the test hooks; the suite loads lib_hooks/"""
    in_child("production", NO_HOOKS, {"CTAMD_LIB_FLAVOUR": "production"}, timeout=300)
