#!/usr/bin/env python3
"""Writes tests/golden/rc64_unchanged_descriptions.json: ctamdDescribePlan of a sample of all-complex128 and all-fp64 contractions, as
the library of the checkout it runs in plans them (no GPU needed).

The file was made once, on the commit BEFORE the mixed fp64 x complex128 kernels (kernels/gett_gen_rc64.inc) and their planner rows
arrived, and tests/test_rc64_planner_cpu.py compares every later library with it: a descriptor that planned before must plan exactly as
it did — same kernel, same index in the kernel table, same description, byte for byte.  Run it again only on a commit whose fp64 /
complex128 plans are meant to change, and say so in that commit.

    python tools/gen_rc64_unchanged_descriptions.py          # needs the built test-hooks libraries (lib_hooks/)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")

OUT = os.path.join(ROOT, "tests", "golden", "rc64_unchanged_descriptions.json")

# id -> (extents, (modesA, modesB, modesC), keyword arguments of ops.contraction_plan beside the data type)
LONE = dict(i=20, j=7, k=50, l=21)
PEEL = dict(a=4, b=3, c=5, d=2, e=6, p=3, q=4, r=2, s=5, t=3, x=4, y=3, z=2)
UNFUSED = dict(a=9, b=7, c=5, d=9, k=37, l=2)
SAMPLE = {}
for _mA, _mB in (("mk", "kn"), ("km", "kn"), ("mk", "nk"), ("km", "nk")):
    for _mC in ("mn", "nm"):
        SAMPLE["ragged_%s_%s_%s" % (_mA, _mB, _mC)] = (dict(m=63, n=45, k=37), (_mA, _mB, _mC), {})
    SAMPLE["even_%s_%s" % (_mA, _mB)] = (dict(m=64, n=48, k=40), (_mA, _mB, "mn"), {})
    SAMPLE["big_%s_%s" % (_mA, _mB)] = (dict(m=2048, n=2048, k=2048), (_mA, _mB, "mn"), {})
SAMPLE["align16"] = (dict(m=64, n=48, k=40), ("km", "kn", "mn"), dict(alignment=16))
SAMPLE["unfused"] = (UNFUSED, ("kabl", "kcdl", "acbdl"), {})
SAMPLE["unfused_long"] = (dict(UNFUSED, k=517), ("kabl", "kcdl", "acbdl"), {})
SAMPLE["splitk"] = (dict(m=128, n=128, k=65536), ("km", "kn", "mn"), {})
SAMPLE["splitk_no_workspace"] = (dict(m=128, n=128, k=65536), ("km", "kn", "mn"), dict(workspace_limit=0))
SAMPLE["batch"] = (dict(i=1024, j=1024, k=256, b=16), ("kib", "kjb", "jib"), {})
SAMPLE["lone"] = (LONE, ("kji", "lk", "li"), {})
SAMPLE["peeled"] = (PEEL, ("paqbrcsdte", "xpyqzrst", "abxcydze"), dict(workspace_limit=1 << 24))
SAMPLE["compute32"] = (dict(m=2048, n=2048, k=2048), ("mk", "kn", "mn"), dict(compute="32F"))
SAMPLE["conj"] = (dict(m=44, n=36, k=28, l=3), ("kml", "nkl", "mnl"), dict(opA=9, opC=9))
DTYPES = ("float64", "complex128")


def describe_all():
    import workspace_cases as wc
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    out = {}
    for dt in DTYPES:
        for cid, (ext, (mA, mB, mC), kw) in SAMPLE.items():
            kw = dict(kw)
            kw.setdefault("workspace_limit", 1 << 28)
            if dt == "float64":
                kw = {k: v for k, v in kw.items() if k not in ("opA", "opC")}      # (conjugation: complex data)
            plan = ops.contraction_plan(h, [ext[c] for c in mA], mA, [ext[c] for c in mB], mB, [ext[c] for c in mC], mC,
                                        dtype=ct.R_64F if dt == "float64" else ct.C_64F, **kw)
            try:
                out["%s_%s" % (dt, cid)] = wc.describe(ct, plan).raw
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
