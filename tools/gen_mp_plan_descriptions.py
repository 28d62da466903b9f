#!/usr/bin/env python3
"""Writes tests/golden/mp_plan_descriptions.json.gz: ctamdMpDescribePlan of every cuTENSORMp contraction plan of the case table
tests/mp_plan_cases.py, for every rank of the case's world — algorithm and byte counts, transfers with their boxes, offsets and pack /
unpack copies, the operands' needed boxes, views, staging and local copies, every field of the reduce plan, every copy's launches and
its single-GPU plan, the local contraction and the byte offset of every workspace region — as the library of the checkout it runs in
plans and describes them, on plan-only handles (no GPU may be visible).  A key is "<case id>/r<rank>"; a plan the library refuses is
recorded as {"status":N}.  The file is the JSON object {key: description}, sorted, gzip-compressed without a time stamp (`zcat` shows it).

The file was made once, on the commit "cuTENSORMg contraction: plan and call as named steps, one piece walk" plus nothing but the
additions to the description itself (per transfer: box, sendOff, recvOff, pack, unpack; operands; reduce; workspace; contractionWs;
contraction) — that is, BEFORE csrc/mp/mp.cpp was split into files and its plan builder and call into named steps — and
tests/test_mp_plan_descriptions_cpu.py compares every later library with it byte for byte.  Run it again only on a commit whose plans or
descriptions are meant to change, and say so in that commit.

    python tools/gen_mp_plan_descriptions.py            # needs the built test-hooks libraries (lib_hooks/)
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")

OUT = os.path.join(ROOT, "tests", "golden", "mp_plan_descriptions.json.gz")


def describe_all(cmp_ct):
    from tests import mp_plan_cases as pc
    out = {}
    for c in pc.CASES:
        out.update(pc.describe_raw(cmp_ct, c))
    return out


def write(out):
    with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        f.write((json.dumps(out, indent=0, sort_keys=True) + "\n").encode())


def read():
    with gzip.open(OUT, "rt") as f:
        return json.load(f)


def main():
    import torch
    assert not torch.cuda.is_available(), "plan-only handles need a host without a GPU"
    from cudalibrarysamples_amd import cutensor as ct
    from cudalibrarysamples_amd import cutensormp
    out = describe_all((cutensormp, ct))
    assert out and all(out.values())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    write(out)
    print("%d descriptions -> %s" % (len(out), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
