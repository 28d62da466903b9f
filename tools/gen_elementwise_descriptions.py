#!/usr/bin/env python3
"""Writes tests/golden/elementwise_descriptions.json.gz: ctamdDescribePlan of every plan of the element-wise and reduction family that the
case tables make (tests/ew_exact_cases.py — all kinds, reductions included —, tests/cplx_trinary_cases.py, tests/convert_cases.py with its
padded case, tests/unary_cases.py), as the library of the checkout it runs in plans and describes them (no GPU needed).  Each table's own
make_plan builds the plans; a key is the table's name, a colon and the case id.  The file is the JSON object {key: description}, sorted,
gzip-compressed without a time stamp (216 KB of text that no one reads line by line; `zcat` shows it).

The file was made once, on the commit BEFORE the execute and describe code of this family moved from host/api.cpp into
host/exec_elementwise.cpp, and tests/test_elementwise_descriptions_cpu.py compares every later library with it byte for byte.  Run it
again only on a commit whose plans or descriptions are meant to change, and say so in that commit.

    python tools/gen_elementwise_descriptions.py            # needs the built test-hooks libraries (lib_hooks/)
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")

OUT = os.path.join(ROOT, "tests", "golden", "elementwise_descriptions.json.gz")


def plans():
    """(key, function of (ct, ops, handle) that makes the plan) for every case of the four tables"""
    import convert_cases as cc
    import cplx_trinary_cases as tc
    import ew_exact_cases as ec
    import unary_cases as uc
    for c in ec.CASES:
        yield "ew_exact_cases:" + c.id, lambda ct, ops, h, c=c: ec.make_plan(ct, ops, h, c)
    for c in tc.CASES:
        yield "cplx_trinary_cases:" + c.id, lambda ct, ops, h, c=c: tc.make_plan(ct, ops, h, c)
    for c in cc.CASES:
        yield "convert_cases:" + c.id, lambda ct, ops, h, c=c: cc.make_plan(ct, ops, h, c)
    yield "convert_cases:" + cc.PAD_CASE.id, lambda ct, ops, h: cc.make_plan(ct, ops, h, cc.PAD_CASE, padding=(cc.PAD_LEFT, cc.PAD_RIGHT, cc.PAD_VALUE))
    for c in uc.CASES:
        yield "unary_cases:" + c.id, lambda ct, ops, h, c=c: uc.make_plan(ct, ops, h, c.base, c.un)


def describe_all(ct, ops, h):
    import workspace_cases as wc
    out = {}
    for key, make in plans():
        assert key not in out, key
        plan = make(ct, ops, h)
        try:
            out[key] = wc.describe(ct, plan).raw
        finally:
            plan.destroy()
    return out


def write(out):
    with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        f.write((json.dumps(out, indent=0, sort_keys=True) + "\n").encode())


def read():
    with gzip.open(OUT, "rt") as f:
        return json.load(f)


def main():
    from cudalibrarysamples_amd import cutensor as ct, ops
    out = describe_all(ct, ops, ops.Handle())
    assert out and all(out.values())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    write(out)
    print("%d descriptions -> %s" % (len(out), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
