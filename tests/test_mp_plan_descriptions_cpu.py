"""ctamdMpDescribePlan of every cuTENSORMp contraction plan of tests/mp_plan_cases.py, for every rank, byte for byte as on the commit before
csrc/mp/mp.cpp was split into files and named steps (tests/golden/mp_plan_descriptions.json.gz, written by
tools/gen_mp_plan_descriptions.py on that commit; plan-only handles, no GPU).  Algorithm, transfers with boxes and offsets, every copy
with its launches and single-GPU plan, operand views and staging, the reduce plan's regions and slots, the local contraction and the
offset of every workspace region: whatever a plan contains is in the description, so a refactoring of the plan builder that changes a
plan fails here."""
import json
import os
import sys

import pytest

from tests import mp_plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cmp_ct(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("the golden descriptions are those of plan-only handles: they need a host without a GPU")
    from cudalibrarysamples_amd import cutensor as ct
    from cudalibrarysamples_amd import cutensormp
    return cutensormp, ct


@pytest.fixture(scope="module")
def golden():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mp_plan_descriptions
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return gen_mp_plan_descriptions.read()


def copies_of(d):
    """every copy of a description: pack / unpack of the transfers, local copies, the reduce plan's"""
    out = [t[k] for t in d["sends"] + d["recvs"] for k in ("pack", "unpack")]
    out += [c for o in d["operands"] or [] for c in o["localCopies"]]
    if d["reduce"]:
        out += [d["reduce"][k] for k in ("cIn", "out", "unpack")] + d["reduce"]["pack"]
    return [c for c in out if c]


def test_the_table_and_the_golden_file_hold_the_same_cases(golden):
    assert sorted(golden) == sorted("%s/r%d" % (c.id, r) for c in pc.CASES for r in range(c.nranks))
    parsed = {k: json.loads(v) for k, v in golden.items()}
    refused = {k for k, d in parsed.items() if "status" in d}
    assert refused == {"limit-subbox-1k/r%d" % r for r in range(4)} | {"limit-cut_n-reduce-1k/r%d" % r for r in range(2)}
    assert all(parsed[k] == {"status": 19} for k in refused)                   # INSUFFICIENT_WORKSPACE
    peeled = {k for k, d in parsed.items() if k not in refused and any(len(c["launches"]) > 1 for c in copies_of(d))}
    assert peeled == {"peeled-gather/r0", "peeled-gather/r1", "peeled-gather-c64/r0", "peeled-gather-c64/r1"}
    assert {d["algorithm"] for k, d in parsed.items() if k not in refused} == {"gather", "reduce"}
    # the contraction's workspace is what the limit leaves after the fixed regions: less than it takes without a limit
    capped, free = parsed["limit-headline-k2-reduce-scratch+%d/r0" % (1 << 20)], parsed["limit-headline-k2-reduce-scratch+%d/r0" % pc.DEFAULT_LIMIT]
    assert 0 < capped["contractionWs"] <= (1 << 20) < free["contractionWs"] and capped["workspace"]["contraction"] == 96 * 96 * 4
    assert any(d.get("compute") is False for d in parsed.values())              # a rank with an empty block of C


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_description_is_unchanged(cmp_ct, golden, case):
    for key, got in pc.describe_raw(cmp_ct, case).items():
        want = golden[key]
        if got != want:
            at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            pytest.fail("%s moved at byte %d: golden ...%s, now ...%s" % (key, at, want[max(0, at - 80):at + 80], got[max(0, at - 80):at + 80]))
