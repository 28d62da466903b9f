#!/usr/bin/env python3
"""Writes tests/golden/contraction_descriptions.json.gz: ctamdDescribePlan's raw text and the required workspace of every contraction,
trinary-contraction and block-sparse plan that the case tables make, as the library of the checkout it runs in plans and describes them
(no GPU needed): tests/workspace_cases.py (the cases that need no switch of the hooks flavour, NO_HOOKS), tests/composite_cases.py (the
trinary contractions and block-sparse cases the library accepts), tests/rc64_cases.py and tests/far_cases.py (the cases that plan in
the calling process; a far case that sweeps a kernel is described at the planner's own choice).  Each table's own make_plan builds the
plans; a key is the table's name, a colon and the case id.  The file is the JSON object {key: [description, required workspace]},
sorted, gzip-compressed without a time stamp (`zcat` shows it).

The file was made once, on the commit BEFORE plan creation, contraction execution and the plan descriptions moved from host/api.cpp into
host/create_plan.cpp, host/exec_contraction.cpp and host/describe.cpp and the plan cache, memo and autotuning state into
host/plan_store.cpp; tests/test_contraction_descriptions_cpu.py compares every later library with it byte for byte.  Descriptions do not
depend on the machine (a handle plans for 256 CUs with and without a device).  Run it again only on a commit whose plans or
descriptions are meant to change, and say so in that commit.

    python tools/gen_contraction_descriptions.py            # needs the built test-hooks libraries (lib_hooks/)
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")

OUT = os.path.join(ROOT, "tests", "golden", "contraction_descriptions.json.gz")
KINDS = ("contraction", "contraction_trinary", "blocksparse")


def plans():
    """(key, function of (ct, ops, handle) that makes the plan) for every case of the four tables"""
    import composite_cases as cc
    import far_cases as fc
    import rc64_cases as rc
    import workspace_cases as wc
    for c in wc.CASES:
        if c.id in wc.NO_HOOKS and c.kind in KINDS:
            yield "workspace_cases:" + c.id, lambda ct, ops, h, c=c: wc.make_plan(ct, ops, h, c)
    for c in cc.CASES:
        if c.kind in KINDS and c.refuse is None:
            yield "composite_cases:" + c.id, lambda ct, ops, h, c=c: cc.make_plan(ct, ops, h, c)
    for cid in rc.IN_PROCESS:
        yield "rc64_cases:" + cid, lambda ct, ops, h, c=rc.BY_ID[cid]: rc.make_plan(ct, ops, h, c)
    for cid in fc.IN_PROCESS:
        yield "far_cases:" + cid, lambda ct, ops, h, c=fc.BY_ID[cid]: fc.make_plan(ct, ops, h, c)


def describe_all(ct, ops, h):
    import workspace_cases as wc
    out = {}
    for key, make in plans():
        assert key not in out, key
        plan = make(ct, ops, h)
        try:
            out[key] = [wc.describe(ct, plan).raw, plan.required_workspace]
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
    assert out and all(d for d, _ in out.values())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    write(out)
    print("%d descriptions -> %s" % (len(out), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
