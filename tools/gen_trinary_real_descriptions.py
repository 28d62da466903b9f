#!/usr/bin/env python3
"""Writes tests/golden/trinary_real_descriptions.json: ctamdDescribePlan of every real-data element-wise trinary case of
tests/ew_exact_cases.py, as the library of the checkout it runs in plans it (no GPU needed).

The file was made once, on the commit BEFORE the complex trinary kernels (kernels/elementwise_trinary_cplx.hip) arrived, and
tests/test_cplx_trinary_cpu.py compares every later library with it: real-data trinary planning must not move.  Run it again only on a
commit whose real-data plans are meant to change, and say so in that commit.

    python tools/gen_trinary_real_descriptions.py            # needs the built test-hooks libraries (lib_hooks/)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")

OUT = os.path.join(ROOT, "tests", "golden", "trinary_real_descriptions.json")


def real_trinary_cases():
    import ew_exact_cases as ec
    return [c for c in ec.CASES if c.kind == "trinary" and c.dtype not in ec.CPLX]


def describe(case):
    import ew_exact_cases as ec
    import workspace_cases as wc
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    plan = ec.make_plan(ct, ops, h, case)
    try:
        return wc.describe(ct, plan).raw
    finally:
        plan.destroy()


def main():
    out = {c.id: describe(c) for c in real_trinary_cases()}
    assert out and all(out.values())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d descriptions -> %s" % (len(out), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
