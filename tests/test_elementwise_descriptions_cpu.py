"""ctamdDescribePlan of every plan of the element-wise and reduction family that the case tables make, byte for byte as on the commit before
the family's execute and describe code moved into host/exec_elementwise.cpp (tests/golden/elementwise_descriptions.json.gz, written by
tools/gen_elementwise_descriptions.py on that commit; no GPU)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_elementwise_descriptions
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return gen_elementwise_descriptions


@pytest.fixture(scope="module")
def described(built, gen):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return gen.describe_all(ct, ops, ops.Handle())


def test_every_table_is_in_the_golden_file_and_nothing_else(described, gen):
    golden = gen.read()
    assert sorted(described) == sorted(golden)
    for table in ("ew_exact_cases", "cplx_trinary_cases", "convert_cases", "unary_cases"):
        assert any(k.startswith(table + ":") for k in golden), table
    assert any('"op":"reduction"' in v for v in golden.values()) and any('"form":"trinary"' in v for v in golden.values())
    assert any('"conj":' in v for v in golden.values()) and any('"unary":' in v for v in golden.values())
    assert any('"convert":' in v for v in golden.values()) and any('"pad":' in v for v in golden.values())


def test_descriptions_are_unchanged(described, gen):
    golden = gen.read()
    moved = {k: (golden[k], v) for k, v in described.items() if golden.get(k) != v}
    assert not moved, "%d descriptions moved, the first: %s" % (len(moved), sorted(moved.items())[0])
