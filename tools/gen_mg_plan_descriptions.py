#!/usr/bin/env python3
"""Writes tests/golden/mg_plan_descriptions.json.gz: ctamdMgDescribePlan of every cuTENSORMg contraction plan of the case table
tests/mg_plan_cases.py — pieces, operand uses, the local contractions with their views, scatter views, wait events, transfers and the
event-block sizes — as the library of the checkout it runs in plans and describes them, on plan-only handles (no GPU may be visible:
device ids 0..7 must stay plan-only).  A key is the case id; a plan the library refuses is recorded as {"status":N}.  The file is the JSON
object {key: description}, sorted, gzip-compressed without a time stamp (`zcat` shows it).

The file was made once, on the commit "Element-wise execute: one launch path for every form and data type" plus nothing but the
additions to the description itself (subs, scatterViews, evPerDevice, evScatter, usesAux, usesComm) — that is, BEFORE csrc/mg/mg.cpp was
split into files and its plan builder and call into named steps — and tests/test_mg_plan_descriptions_cpu.py compares every later
library with it byte for byte.  Run it again only on a commit whose plans or descriptions are meant to change, and say so in that commit.

    python tools/gen_mg_plan_descriptions.py            # needs the built test-hooks libraries (lib_hooks/)
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")

OUT = os.path.join(ROOT, "tests", "golden", "mg_plan_descriptions.json.gz")


def describe_all(cm):
    from tests import mg_plan_cases as pc
    return {c.id: pc.describe_raw(cm, c) for c in pc.CASES}


def write(out):
    with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        f.write((json.dumps(out, indent=0, sort_keys=True) + "\n").encode())


def read():
    with gzip.open(OUT, "rt") as f:
        return json.load(f)


def main():
    import torch
    assert not torch.cuda.is_available(), "plan-only handles need a host without a GPU"
    from cudalibrarysamples_amd import cutensormg as cm
    out = describe_all(cm)
    assert out and all(out.values())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    write(out)
    print("%d descriptions -> %s" % (len(out), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
