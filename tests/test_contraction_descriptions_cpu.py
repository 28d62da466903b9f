"""ctamdDescribePlan and the required workspace of every contraction, trinary-contraction and block-sparse plan that the case tables make,
byte for byte as on the commit before plan creation, contraction execution and the descriptions moved out of host/api.cpp and the plan
cache, memo and autotuning state into host/plan_store.cpp (tests/golden/contraction_descriptions.json.gz, written by
tools/gen_contraction_descriptions.py on that commit; no GPU)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_contraction_descriptions
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return gen_contraction_descriptions


@pytest.fixture(scope="module")
def described(built, gen):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return gen.describe_all(ct, ops, ops.Handle())


def test_every_table_is_in_the_golden_file_and_nothing_else(described, gen):
    import workspace_cases as wc
    golden = gen.read()
    assert sorted(described) == sorted(golden)
    for table in ("workspace_cases", "composite_cases", "rc64_cases", "far_cases"):
        assert any(k.startswith(table + ":") for k in golden), table
    kinds = {c.id: c.kind for c in wc.CASES}
    assert sorted(k.split(":")[1] for k in golden if k.startswith("workspace_cases:")) == sorted(i for i in wc.NO_HOOKS if kinds[i] in gen.KINDS)
    text = [d for d, _ in golden.values()]
    for path in ('"op":"contraction"', '"op":"contraction_trinary"', '"op":"blocksparse"', '"lone_reduce_A":1', '"peeled_modes":',
                 '"kname":"gett_wide_kernel"', '"kname":"gett_f32_stream_kernel"', '"family":1', '"family":2', '"real":'):
        assert any(path in d for d in text), path
    assert any(ws > 0 for _, ws in golden.values())


def test_descriptions_and_workspaces_are_unchanged(described, gen):
    golden = gen.read()
    moved = {k: (golden[k], v) for k, v in described.items() if golden.get(k) != v}
    assert not moved, "%d plans moved, the first: %s" % (len(moved), sorted(moved.items())[0])
