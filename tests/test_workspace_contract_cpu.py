"""The workspace contract of every plan kind on the CPU planner (no GPU): estimate -> plan -> required_workspace at each of
CUTENSOR_WORKSPACE_MIN / DEFAULT / MAX, and plans at small and odd limits, for every case of tests/workspace_cases.py.

- A plan created at a preference's estimate succeeds and requires at most that estimate (cuTENSOR/contraction.cu:207-239).  At MIN
  too: the reference's binding re-plans at WORKSPACE_MIN after an allocation failure (cuTENSOR/python/cutensor/torch/einsum.cc:110).
- estimate(MIN) <= estimate(DEFAULT) <= estimate(MAX).
- At any limit a plan either fits into it or is refused with INSUFFICIENT_WORKSPACE, and only below estimate(MIN).
- The same on a handle with the plan memo, planned from the large limit down: the memo is keyed by the limit, so a small-limit plan
  must not inherit a large-limit requirement.
- The DEFAULT and MAX estimates agree with the plan created at the preference's cap (workspace_cases.check_agreement): equal, except
  under the best-four policy of the fp32 ranked list, where the estimate bounds the requirement.  CORNERS are problems on which the
  estimate once took another route than the plan.
A case whose switch the library reads once per process (Case.fresh) is planned in a child process started with it."""
import pytest

from workspace_cases import CASES, CORNERS, corner_contract, in_child, memo_contract, plan_contract


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_estimate_plan_and_required_at_every_preference(env, case):
    ct, ops = env
    if case.fresh:
        in_child("plan", [case.id], case.env, timeout=120)
    else:
        plan_contract(ct, ops, case)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_plan_memo_is_keyed_by_the_limit(env, case):
    ct, ops = env
    if case.fresh:
        in_child("memo", [case.id], case.env, timeout=120)
    else:
        memo_contract(ct, ops, case)


@pytest.mark.parametrize("corner", CORNERS, ids=[c.id for c in CORNERS])
def test_estimate_takes_the_route_of_the_plan(env, corner):
    ct, ops = env
    corner_contract(ct, ops, corner)
