"""ctamdMgDescribePlan of every cuTENSORMg contraction plan of tests/mg_plan_cases.py, byte for byte as on the commit before csrc/mg/mg.cpp
was split into files and named steps (tests/golden/mg_plan_descriptions.json.gz, written by tools/gen_mg_plan_descriptions.py on that
commit; plan-only handles, no GPU).  Pieces, local contractions and their views, wave and event numbers, transfers in order: whatever a
plan contains is in the description, so a refactoring of the plan builder that changes a plan fails here."""
import os
import sys

import pytest

from tests import mg_plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cm(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("plan-only handles for device ids 0..7 need a host without that many GPUs")
    from cudalibrarysamples_amd import cutensormg
    return cutensormg


@pytest.fixture(scope="module")
def golden():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mg_plan_descriptions
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return gen_mg_plan_descriptions.read()


def test_the_table_and_the_golden_file_hold_the_same_cases(golden):
    assert sorted(golden) == sorted(c.id for c in pc.CASES)
    assert golden["ragged_contracted-k176-bf16"] == '{"status":15}'       # NOT_SUPPORTED: 16-bit data never accumulates through D
    assert any('"peeled":0' not in v for v in golden.values()) and any('"acc":1' in v for v in golden.values())


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_description_is_unchanged(cm, golden, case):
    got = pc.describe_raw(cm, case)
    want = golden[case.id]
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail("%s moved at byte %d: golden ...%s, now ...%s" % (case.id, at, want[max(0, at - 80):at + 80], got[max(0, at - 80):at + 80]))
