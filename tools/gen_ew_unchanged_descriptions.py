#!/usr/bin/env python3
"""Writes tests/golden/many_modes_unchanged_descriptions.json: ctamdDescribePlan of every permutation, binary, trinary and reduction case
of tests/ew_exact_cases.py and tests/convert_cases.py, as the library of the checkout it runs in plans them (no GPU needed).

The file was made once, on the commit BEFORE the mode-table kernels (kernels/elementwise_table.hip) and their planner
(host/plan_elementwise_table.cpp) arrived, and tests/test_many_modes_cpu.py compares every later library with it: the mode-table route
starts only where the planner used to refuse a problem for its mode count, so a problem that planned before must plan exactly as it did —
same variant, same tiles, same description, byte for byte.  Run it again only on a commit whose element-wise or reduction plans are meant
to change, and say so in that commit.

    python tools/gen_ew_unchanged_descriptions.py          # needs the built test-hooks libraries (lib_hooks/)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")

OUT = os.path.join(ROOT, "tests", "golden", "many_modes_unchanged_descriptions.json")


def describe_all():
    import convert_cases as cv
    import ew_exact_cases as ew
    import workspace_cases as wc
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    out = {}
    for mod, prefix in ((ew, "ew:"), (cv, "convert:")):
        for case in mod.CASES:
            with wc.hook_env(case):
                plan = mod.make_plan(ct, ops, h, case)
            try:
                out[prefix + case.id] = wc.describe(ct, plan).raw
            finally:
                plan.destroy()
    return out


def main():
    out = describe_all()
    assert out and all(out.values())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d descriptions -> %s" % (len(out), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
